"""The scenes of the forward compositor's branch tests, shared by tests/test_forward_check.py (the
oracle alone, CPU) and tests/test_forward_branches_gpu.py (every forward instantiation against it,
through lsr_testutil.image_check).

The cases named as in bwd_cases (A, B, E, F, G, P, L7, L32) are those scenes unchanged, oracle runs
shared.  (Its scenes C, D and H have no wholly saturated quadrant, see below: their channel counts
1, 16 and 64 are cases C1, C16 and C64 here, on seeds that have one.)
The others put further channel counts on bwd_cases' base scene (83 x 61, 1500 Gaussians: culled
rows, capped alphas, clamped colours, quadrants wholly outside the image), so that every
instantiation of the forward kernels stages its language rows both ways:

    kernel                          staging                    cases (C)
    k_render_fwd_wave<0>            none                       A (0), N6 (6, include_feature=False)
    k_render_fwd_wave<4>            float4 / scalar            C4 (4) / C1 (1)
    k_render_fwd_wave<8>            float4 / scalar            P (8) / B (5)
    k_render_fwd_wave<16>           float4 / scalar            C16 (16) / C12 (12)
    k_render_fwd_wave<64>           float4 / scalar            C64 (64) / C33 (33), G (48), C63 (63)
    k_render_fwd_wave_mfma<false>   float4 / masked scalar     F (32) / E (17), C24 (24), C31 (31)
    k_render_fwd_wave_mfma<true>    pre-split operands         F (32) through preprocess_views_native

and add three scenes:

  S7, S32   long and saturating: bwd_cases' long scene (6000 wide Gaussians over 35 x 19, lists of
            up to 4098 entries) with the opacities x 0.2 instead of x 0.05.  Every pixel then stops
            (T (1 - alpha) < 1e-4) between entry 409 and entry 2872 of its list: the wave fills its
            128-entry FIFO many times and leaves through __all(done) with entries still queued and
            unscanned.  At x 0.05 no pixel stops.
  HE        half empty: 800 small Gaussians (no wide ones) over 83 x 61, all moved to x >= 0.15 z,
            the right half of the image: 12 of the 24 tiles have no entry (their ranges are the
            preset (~0, 0) until the compositor rewrites them), and the tiles beside them have
            pixels no Gaussian reaches.
  W5, W32   views: 3 cameras of the base scene composited by one launch whose grid row selects the
            view (preprocess_views_native + binning_views_native + render_views_native); the middle
            camera is moved 1000 units back so that it sees nothing.  C = 5 (k_render_fwd_wave<8>,
            scalar staging) and C = 32 with pre-split operands (k_render_fwd_wave_mfma<true>).

New base-scene cases take their seed from those bwd_cases found usable (0, 1, 7: at least 32
capped pairs), and of those one at which the scene also has an 8 x 8 quadrant all of whose pixels
saturate before their list ends (final_T < 1e-2, the last contributor not the list's last entry),
and at least 500 such pixels; check_preconditions asserts it.
"""
import dataclasses
import functools

import numpy as np

import bwd_cases
import synthetic
from bwd_cases import BG
from helpers import small_case
from lsr_testutil import run_oracle

S_OPACITY = 0.2

# kernel / staging: what the case must reach (kernel_of checks it against the launchers' rules)
CASES = {
    "A": dict(bwd="A", kernel="wave<0>", staging="none"),
    "N6": dict(seed=1, C=6, include_feature=False, kernel="wave<0>", staging="none"),
    "C4": dict(seed=0, C=4, kernel="wave<4>", staging="float4"),
    "C1": dict(seed=0, C=1, sh_degree=2, kernel="wave<4>", staging="scalar"),
    "P": dict(bwd="P", kernel="wave<8>", staging="float4"),
    "B": dict(bwd="B", kernel="wave<8>", staging="scalar"),
    "C16": dict(seed=1, C=16, kernel="wave<16>", staging="float4"),
    "C12": dict(seed=1, C=12, kernel="wave<16>", staging="scalar"),
    "C64": dict(seed=0, C=64, sh_degree=1, kernel="wave<64>", staging="float4"),
    "G": dict(bwd="G", kernel="wave<64>", staging="scalar"),
    "C33": dict(seed=0, C=33, kernel="wave<64>", staging="scalar"),
    "C63": dict(seed=1, C=63, sh_degree=2, kernel="wave<64>", staging="scalar"),
    "F": dict(bwd="F", kernel="mfma<false>", staging="float4"),
    "E": dict(bwd="E", kernel="mfma<false>", staging="scalar"),
    "C24": dict(seed=0, C=24, kernel="mfma<false>", staging="scalar"),
    "C31": dict(seed=1, C=31, sh_degree=1, kernel="mfma<false>", staging="scalar"),
    "L7": dict(bwd="L7", kernel="wave<8>", staging="scalar"),
    "L32": dict(bwd="L32", kernel="mfma<false>", staging="float4"),
    "S7": dict(saturating=True, C=7, kernel="wave<8>", staging="scalar"),
    "S32": dict(saturating=True, C=32, kernel="mfma<false>", staging="float4"),
    "HE": dict(half_empty=True, C=5, kernel="wave<8>", staging="scalar"),
    "W5": dict(seed=1, C=5, views=3, kernel="wave<8>", staging="scalar"),
    "W32": dict(seed=0, C=32, views=3, split=True, kernel="mfma<true>", staging="pre-split"),
}
# bwd_cases' scenes that are no case here (C, D and H have no wholly saturated quadrant; V16, V64): the backward
# module puts their forwards through image_check too, so case(), reference() and lang_scale() take them
BWD_ONLY = [n for n in bwd_cases.CASES if n not in CASES]


def kernel_of(C, include_feature=True, split=False):
    """(kernel, staging) the forward launchers choose (launch_render_fwd_wave_views, lang_pad)."""
    C = C if include_feature else 0
    pad = 0 if C == 0 else 4 if C <= 4 else 8 if C <= 8 else 16 if C <= 16 else 32 if C <= 32 else 64
    if pad == 0:
        return "wave<0>", "none"
    if pad == 32:
        if split and C == 32:
            return "mfma<true>", "pre-split"
        return "mfma<false>", "float4" if C == 32 else "scalar"
    return f"wave<{pad}>", "float4" if C == pad else "scalar"


class Case:
    """bwd_cases.Case's fields as far as the forward needs them, and include_feature, split (the
    pre-split language operands) and kind: base, long, saturating, half_empty."""

    def __init__(self, name):
        spec = CASES.get(name) or dict(bwd=name)    # any other scene of bwd_cases, as it is there
        self.name, self.bwd = name, spec.get("bwd")
        self.empty_view = 1 if spec.get("views") else None
        self.include_feature = spec.get("include_feature", True)
        self.split = spec.get("split", False)
        self.precomp = self.cov3D = False
        self.colors = None
        self.sh_degree, self.scale_modifier = spec.get("sh_degree", 3), spec.get("scale_modifier", 1.0)
        if "bwd" in spec:
            b = bwd_cases.case(spec["bwd"])
            self.C, self.W, self.H, self.scene, self.cams = b.C, b.W, b.H, b.scene, b.cams
            self.sh_degree, self.scale_modifier = b.sh_degree, b.scale_modifier
            self.precomp, self.cov3D, self.colors = b.precomp, b.cov3D, b.colors
            self.kind = "long" if b.long else "base"
        elif spec.get("saturating"):
            self.C, self.W, self.H, self.kind = spec["C"], bwd_cases.LONG_W, bwd_cases.LONG_H, "saturating"
            self.scene, cam = bwd_cases.long_scene(self.C, opacity=S_OPACITY)
            self.cams = [cam]
        elif spec.get("half_empty"):
            self.C, self.W, self.H, self.kind = spec["C"], bwd_cases.BASE_W, bwd_cases.BASE_H, "half_empty"
            self.scene, cam = small_case(P=800, W=self.W, H=self.H, C=self.C, seed=3, big_frac=0.0)
            m = self.scene.means3D
            m[:, 0] = m[:, 0].abs() + 0.15 * m[:, 2]
            self.cams = [cam]
        else:
            self.C, self.W, self.H, self.kind = spec["C"], bwd_cases.BASE_W, bwd_cases.BASE_H, "base"
            self.scene, cam = bwd_cases.base_scene(spec["seed"], self.C)
            self.cams = [cam]
            if spec.get("views"):
                self.cams = synthetic.camera_batch(spec["views"], self.W, self.H, seed=31)
                away = self.cams[1].world_view_transform.clone()
                away[3, 2] -= 1000.0           # the middle view: every Gaussian behind the near plane
                self.cams[1] = dataclasses.replace(self.cams[1], world_view_transform=away)
        self.long = self.kind in ("long", "saturating")   # bwd_cases.view_figures reads it
        if name in CASES:
            assert kernel_of(self.C, self.include_feature, self.split) == (spec["kernel"], spec["staging"]), name

    def run_kw(self):
        """keywords of lsr_testutil.run_native / run_oracle"""
        return dict(bg=BG, sh_degree=self.sh_degree, scale_modifier=self.scale_modifier,
                    use_precomp_cov=self.cov3D, colors_precomp=self.colors, include_feature=self.include_feature)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


@functools.lru_cache(maxsize=None)
def reference(name, double=False):
    """The oracle's forward of each view (a list of OracleResult).  Computed once per case and
    precision; shared, never modified."""
    c = case(name)
    if c.bwd:
        return bwd_cases.reference(c.bwd, double).views
    return [run_oracle(c.scene, cam, double=double, **c.run_kw()) for cam in c.cams]


@functools.lru_cache(maxsize=None)
def lang_scale(name):
    """Per view the language image's rounding scale A [C, H, W]: the double oracle's forward with
    the language rows replaced by their magnitudes.  The weights alpha T do not depend on the rows,
    so this is the sum of |f| w over the pixel's blended entries.  None where the forward writes no
    language (C = 0, include_feature=False: the image must then be exactly 0)."""
    c = case(name)
    if not (c.C and c.include_feature):
        return [None for _ in c.cams]
    mag = np.abs(c.scene.lang.numpy())
    return [run_oracle(c.scene, cam, double=True, lang=mag, **c.run_kw()).lang for cam in c.cams]


def saturated_pixels(ref_view, W, H):
    """[H, W] bool: final_T < 1e-2 and the last contributor lies before the end of the tile's list:
    the pixel has all but stopped with entries still behind it."""
    st = ref_view.state()
    rr, gx = st["ranges"].astype(np.int64), (W + 15) // 16
    length = np.zeros((H, W), np.int64)
    for t in range(len(rr)):
        length[16 * (t // gx):16 * (t // gx) + 16, 16 * (t % gx):16 * (t % gx) + 16] = rr[t, 1] - rr[t, 0]
    return (st["final_T"] < 1e-2) & (st["n_contrib"] < length)


def stopped_pixels(ref_view, W, H):
    """[H, W] bool: the pixel left its list through T (1 - alpha) < 1e-4 (the kernels' `done`), i.e.
    some entry behind its last contributor still passes the alpha tests (it would have been blended
    otherwise).  Evaluated in fp64 from the oracle's xy and conic_o as bwd_cases.capped_pairs does,
    with a 1e-5 margin on the 1/255 threshold so that no borderline alpha counts."""
    st = ref_view.state()
    xy, co = st["xy"].astype(np.float64), st["conic_o"].astype(np.float64)
    pl, rr, nc = st["point_list"].astype(np.int64), st["ranges"], st["n_contrib"]
    gx = (W + 15) // 16
    out = np.zeros((H, W), bool)
    for t in range(len(rr)):
        g = pl[rr[t, 0]:rr[t, 1]]
        if len(g) == 0:
            continue
        tx, ty = t % gx, t // gx
        px, py = np.meshgrid(np.arange(16 * tx, min(16 * tx + 16, W)), np.arange(16 * ty, min(16 * ty + 16, H)))
        px, py = px.ravel(), py.ravel()
        dx = xy[g, 0][:, None] - px[None].astype(np.float64)
        dy = xy[g, 1][:, None] - py[None].astype(np.float64)
        a, b, c, o = (co[g, k][:, None] for k in range(4))
        power = -0.5 * (a * dx * dx + c * dy * dy) - b * dx * dy
        alpha = np.minimum(0.99, o * np.exp(np.minimum(power, 0.0)))
        behind = np.arange(len(g))[:, None] >= nc[py, px][None].astype(np.int64)
        out[py, px] = (behind & (power <= 0) & (alpha >= (1.0 / 255.0) * (1 + 1e-5))).any(axis=0)
    return out


def quadrants(W, H):
    """(tile, y slice, x slice) of every 8 x 8 quadrant with a pixel inside the image."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    return [(ty * gx + tx, slice(y0, min(y0 + 8, H)), slice(x0, min(x0 + 8, W)))
            for ty in range(gy) for tx in range(gx) for y0 in (16 * ty, 16 * ty + 8) for x0 in (16 * tx, 16 * tx + 8)
            if y0 < H and x0 < W]


def check_preconditions(name):
    """What each scene must exercise, asserted on the float oracle's state (so that a scene cannot
    silently stop reaching its branch).  Returns the measured figures per view."""
    c = case(name)
    out = {}
    for v, r in enumerate(reference(name)):
        st = r.state()
        nc, rr = st["n_contrib"], st["ranges"].astype(np.int64)
        if v == c.empty_view:     # the view that sees nothing
            assert r.num_rendered == 0 and (r.radii == 0).all() and (nc == 0).all(), name
            out[v] = dict(num_rendered=0)
            continue
        sat, stopped = saturated_pixels(r, c.W, c.H), stopped_pixels(r, c.W, c.H)
        quads = quadrants(c.W, c.H)
        whole = [q for q in quads if sat[q[1], q[2]].all()]
        fig = dict(saturated_pixels=int(sat.sum()), saturated_quadrants=len(whole), quadrants=len(quads),
                   stopped_pixels=int(stopped.sum()), min_n_contrib=int(nc.min()), max_n_contrib=int(nc.max()))
        if c.kind == "half_empty":
            empty = rr[:, 0] == rr[:, 1]
            gx = (c.W + 15) // 16
            partly = [t for t in np.nonzero(~empty)[0]
                      if (nc[16 * (t // gx):16 * (t // gx) + 16, 16 * (t % gx):16 * (t % gx) + 16] == 0).any()]
            fig.update(empty_tiles=int(empty.sum()), nonempty_tiles=int((~empty).sum()),
                       nonempty_tiles_with_uncovered_pixels=len(partly), uncovered_pixels=int((nc == 0).sum()),
                       visible=int((r.radii > 0).sum()))
            assert fig["empty_tiles"] >= 6 and fig["nonempty_tiles"] >= 6 and partly, (name, fig)
        else:
            fig.update(bwd_cases.view_figures(c, r, (name, v)))
            if c.kind == "saturating":
                # every pixel leaves through `done`, the list not at its end: the waves' __all(done) exit
                assert len(whole) == len(quads) and stopped.all() and fig["max_n_contrib"] > 1024, (name, fig)
            elif c.kind == "base":
                assert len(whole) >= 1 and fig["saturated_pixels"] >= 500, (name, v, fig)
        out[v] = fig
    return out
