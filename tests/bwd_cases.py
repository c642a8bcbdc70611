"""The scenes of the backward compositor's branch tests, shared by tests/test_backward_check.py (the
oracle alone, CPU) and tests/test_backward_branches_gpu.py (every kernel branch against it).

Base scene: small_case(P=1500, 83 x 61, big_frac=0.05).  83 x 61 is 6 x 4 tiles whose last column
is 3 px wide (its right quadrants lie wholly outside the image) and whose last row is 13 px high
(its lower quadrants are partial).  Edits: the first 40 Gaussians behind the camera (culled), every
9th opacity 0.999 and its scales x3 (alphas above the 0.99 cap), every 3rd Gaussian's SH DC lowered by 1.5 (about a
tenth of the visible colour channels clamped at 0).  Long scene (cases L*): 6000 wide Gaussians over
35 x 19 (3 x 2 tiles; the edge tiles' right and lower quadrants wholly outside) with the opacities
scaled by L_OPACITY, so that pixels saturate late: the largest n_contrib exceeds 1024, at least 8
fills of the wave kernel's 128-entry FIFO.  Upstream gradients are standard normal for colour,
language and depth; the background is (0.3, 0.6, 0.9).

Preprocess-backward scenes (PP_CASES, tests/test_preprocess_bwd_branches_gpu.py): the base scene's
edits on PP_P = 700 Gaussians -- three 256-row blocks of the per-Gaussian kernel, the last one
partial (188 rows), the first one holding the 40 culled rows next to visible ones -- with 3 language
channels and the launcher branch under test: M SH coefficients per Gaussian (the first M of the
scene's 16 at the degree they allow; M = 25 appends 9 rows the degree-3 colour never reads),
colors_precomp instead of SH, or cov3D_precomp instead of scales and rotations.

Two more scenes on the same 700 Gaussians with M = 16 (PP_EXTRA, explicit seeds: the seeds of
PP_CASES come from the sorted names and must not move) reach the geometry branches no random scene
does.  CLAMP (forward and backward): rows 40..87 are wide Gaussians (scales 0.25..0.75) at depth
2..5 placed 1.35..1.85 tan(fov) z off the axis, alternately in x and in y -- outside the 1.3 tan(fov)
clamp of the EWA projection yet reaching into the image, so the forward clamps t and the backward
zeroes that Jacobian column; rows 100..149 carry five copies of FAINT_OPACITIES, around the
opacity exp(-1e-3) / 255 below which no pixel can pass the alpha prefilter: such a Gaussian keeps
its radius and is not listed (five copies: with four, 15 of the 16 rows of opacity <= 0.003 are
visible, one short of what check_preprocess_preconditions asserts).  NEAR (forward only) adds six rows on the optical axis of the origin
camera (identity view matrix: the view-space z is the stored one exactly) at and beside the near
plane z = 0.2f; three are culled, three kept.  In double 0.2f > 0.2, the splats at z = 0.2f become
visible and cover the image: NEAR has no meaning against the double oracle or in a backward test.
"""
import functools

import numpy as np
import torch

import oracle
import synthetic
from helpers import oracle_settings, small_case

BG = (0.3, 0.6, 0.9)
BASE_W, BASE_H = 83, 61
LONG_W, LONG_H = 35, 19
L_OPACITY = 0.05   # found on the oracle: already at 0.05 the largest n_contrib is 4098, the whole list
# An opacity of 0.999 caps alpha only within 0.13 sigma of a centre, and the scene's splats are
# mostly under a pixel wide: with the opacity edit alone the oracle counts 1 to 16 capped
# (Gaussian, pixel) pairs per scene over seeds 0..23 (scale_modifier 1 and 0.7; three cameras),
# never the 20 the tests require.  The capped
# Gaussians are therefore also made 3x wider, and the seeds are the ones (of 0..7) at which every
# camera and scale_modifier in use then has at least 32 pairs; check_preconditions asserts it.
# (Case D is not on seed 0: at scale_modifier 0.7 one means2D element of that scene moves by
# 1.2e-4 A between the float and the double oracle, more than the bound grants the kernels.)

# C: language channels; views: cameras of a camera_batch (else the origin camera); precomp:
# cov3D_precomp + colors_precomp instead of scales / rotations / SH
CASES = {
    "A": dict(seed=0, C=0, sh_degree=0),
    "B": dict(seed=1, C=5),
    "C": dict(seed=7, C=1, sh_degree=2),
    "D": dict(seed=1, C=16, scale_modifier=0.7),
    "E": dict(seed=7, C=17, scale_modifier=1.6, sh_degree=1),
    "F": dict(seed=0, C=32),
    "G": dict(seed=1, C=48),
    "H": dict(seed=7, C=64, scale_modifier=0.7, sh_degree=1),
    "P": dict(seed=0, C=8, precomp=True),
    "L7": dict(C=7, long=True),
    "L32": dict(C=32, long=True),
    "V16": dict(seed=1, C=16, views=2),
    "V64": dict(seed=7, C=64, views=2),
}


PP_P = 700
PP_CASES = {
    "M1": dict(M=1, sh_degree=0),
    "M4": dict(M=4, sh_degree=1),
    "M9": dict(M=9, sh_degree=2),
    "M16": dict(M=16),
    "M25": dict(M=25),
    "COL": dict(colors=True),
    "COV": dict(cov3D=True),
}


# opacities around t = exp(-1e-3) / 255, skip_power's switch: at and below it no pixel passes 1 / 255
_T = np.float32(np.exp(-1e-3) / 255.0)
FAINT_OPACITIES = np.array([0.0, 1e-6, 0.001, 0.003, np.nextafter(_T, np.float32(0)), np.nextafter(_T, np.float32(1)),
                            1.0 / 255.0, 0.004, 0.005, 0.01], np.float32)
CLAMP_ROWS, FAINT_ROWS, NEAR_ROWS = slice(40, 88), slice(100, 150), slice(200, 206)
NEAR_Z = np.array([0.2, 0.2, np.nextafter(np.float32(0.2), np.float32(1)), 0.21, 0.19999, 0.25], np.float32)
NEAR_KEPT = NEAR_Z > np.float32(0.2)
PP_EXTRA = {
    "CLAMP": dict(M=16, case_seed=107, clamp=True),
    "NEAR": dict(M=16, case_seed=108, clamp=True, near=True),
}


def pp_spec(name):
    return PP_CASES[name] if name in PP_CASES else PP_EXTRA[name]


def clamp_edits(sc, cam, near=False):
    """The CLAMP (and NEAR) rows written into a base scene (module docstring)."""
    g = torch.Generator().manual_seed(5)
    n = CLAMP_ROWS.stop - CLAMP_ROWS.start
    z = torch.rand(n, generator=g) * 3.0 + 2.0
    off = (torch.rand(n, generator=g) * 0.5 + 1.35) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
    inside = torch.rand(n, generator=g) * 1.6 - 0.8
    even = torch.arange(n) % 2 == 0
    x = torch.where(even, off, inside) * cam.tanfovx * z
    y = torch.where(even, inside, off) * cam.tanfovy * z
    sc.means3D[CLAMP_ROWS] = torch.stack([x, y, z], dim=1)
    sc.scales[CLAMP_ROWS] = torch.rand(n, 3, generator=g) * 0.5 + 0.25
    sc.opacities[FAINT_ROWS] = torch.from_numpy(np.tile(FAINT_OPACITIES, 5)).reshape(-1, 1)
    if near:
        assert np.array_equal(cam.world_view_transform.numpy(), np.eye(4, dtype=np.float32))
        xy = torch.tensor([[0.0, 0.0], [0.004, 0.0], [0.0, 0.004], [-0.004, 0.0], [0.0, -0.004], [0.004, 0.004]])
        sc.means3D[NEAR_ROWS] = torch.cat([xy, torch.from_numpy(NEAR_Z)[:, None]], dim=1)


def base_scene(seed, C, P=1500):
    """The base scene and its origin camera (module docstring: culled, capped, clamped edits)."""
    sc, cam = small_case(P=P, W=BASE_W, H=BASE_H, C=C, seed=seed, big_frac=0.05)
    sc.means3D[:40, 2] = -1.0
    sc.opacities[::9] = 0.999
    sc.scales[::9] *= 3.0
    sc.shs[::3, 0, :] -= 1.5
    return sc, cam


def long_scene(C, opacity=L_OPACITY):
    """The long scene and its origin camera, the opacities scaled by `opacity`."""
    sc, cam = small_case(P=6000, W=LONG_W, H=LONG_H, C=C, seed=12, logscale_mean=-1.5, big_frac=0.0)
    sc.opacities *= opacity
    return sc, cam


class Case:
    def __init__(self, name):
        pp = name in PP_CASES or name in PP_EXTRA
        spec = dict(seed=1, C=3, **pp_spec(name)) if pp else CASES[name]
        self.name, self.C = name, spec["C"]
        self.sh_degree = spec.get("sh_degree", 3)
        self.scale_modifier = spec.get("scale_modifier", 1.0)
        self.long, self.precomp = spec.get("long", False), spec.get("precomp", False)
        self.cov3D = self.precomp or spec.get("cov3D", False)
        if "case_seed" in spec:
            seed = spec["case_seed"]
        else:
            seed = 100 + sorted(PP_CASES).index(name) if pp else sorted(CASES).index(name)
        if self.long:
            self.W, self.H = LONG_W, LONG_H
            sc, cam = long_scene(self.C)
        else:
            self.W, self.H = BASE_W, BASE_H
            sc, cam = base_scene(spec["seed"], self.C, P=PP_P if pp else 1500)
            M = spec.get("M", 16)
            if M != 16:
                extra = torch.randn(sc.P, max(M - 16, 0), 3, generator=torch.Generator().manual_seed(seed)) * 0.1
                sc.shs = torch.cat([sc.shs[:, :M], extra], dim=1).contiguous()
            if spec.get("clamp"):
                clamp_edits(sc, cam, near=spec.get("near", False))
        self.scene = sc
        nv = spec.get("views", 0)
        self.cams = synthetic.camera_batch(nv, self.W, self.H, seed=31) if nv else [cam]
        rng = np.random.default_rng(700 + seed)
        self.colors = rng.uniform(0, 1, (sc.P, 3)).astype(np.float32) if self.precomp or spec.get("colors") else None
        shape = (self.H, self.W)
        self.gcol = [rng.normal(size=(3,) + shape).astype(np.float32) for _ in self.cams]
        self.glang = [rng.normal(size=(self.C,) + shape).astype(np.float32) if self.C else None for _ in self.cams]
        self.gdep = [rng.normal(size=(1,) + shape).astype(np.float32) for _ in self.cams]

    def run_kw(self):
        """keywords of lsr_testutil.run_native / run_oracle"""
        return dict(bg=BG, sh_degree=self.sh_degree, scale_modifier=self.scale_modifier,
                    use_precomp_cov=self.cov3D, colors_precomp=self.colors)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


class Reference:
    """The oracle's forward of each view and its backward summed over the views (float64 arrays):
    grads, and abs (the abs_terms sums of the direct fields: each element's rounding scale A)."""

    def __init__(self, c, double):
        sc = c.scene
        self.views = []
        self.grads = self.abs = None
        for v, cam in enumerate(c.cams):
            s = oracle_settings(cam, bg=BG, sh_degree=c.sh_degree, scale_modifier=c.scale_modifier)
            kw = {}
            if c.cov3D:
                kw["cov3D_precomp"] = oracle.cov3d(sc.scales.numpy(), sc.rotations.numpy())
            else:
                kw["scales"], kw["rotations"] = sc.scales.numpy(), sc.rotations.numpy()
            if c.colors is not None:
                kw["colors_precomp"] = c.colors
            else:
                kw["shs"] = sc.shs.numpy()
            r = oracle.forward(s, sc.means3D.numpy(), sc.opacities.numpy(), lang=sc.lang.numpy() if c.C else None,
                               double=double, **kw)
            g = r.backward(c.gcol[v], c.glang[v], c.gdep[v][0])
            ab = r.backward(c.gcol[v], c.glang[v], c.gdep[v][0], abs_terms=True)
            g = {k: x.astype(np.float64) for k, x in g.items()}
            ab = {k: ab[k].astype(np.float64) for k in ("lang", "opacity", "means2D")}
            self.grads = g if self.grads is None else {k: self.grads[k] + g[k] for k in g}
            self.abs = ab if self.abs is None else {k: self.abs[k] + ab[k] for k in ab}
            self.views.append(r)


@functools.lru_cache(maxsize=None)
def reference(name, double=False):
    """Computed once per case and precision; shared, never modified."""
    return Reference(case(name), double)


def capped_pairs(ref_view, W, H):
    """(Gaussian, pixel) pairs among the pixels' contributors whose uncapped alpha o exp(power)
    exceeds 0.99, evaluated in fp64 from the oracle's xy and conic_o (as
    lsr_testutil.check_binning_against_upstream evaluates alpha)."""
    st = ref_view.state()
    xy, co = st["xy"].astype(np.float64), st["conic_o"].astype(np.float64)
    pl, rr, nc = st["point_list"].astype(np.int64), st["ranges"], st["n_contrib"]
    gx = (W + 15) // 16
    n = 0
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
        blended = np.arange(len(g))[:, None] < nc[py, px][None].astype(np.int64)
        n += int((blended & (power <= 0) & (o * np.exp(np.minimum(power, 0.0)) > 0.99)).sum())
    return n


def outside_quadrant_tiles(ref_view, W, H):
    """Tiles with a non-empty list and a quadrant wholly outside the image."""
    rr = ref_view.state()["ranges"]
    gx = (W + 15) // 16
    return [t for t in range(len(rr)) if rr[t, 1] > rr[t, 0] and
            (16 * (t % gx) + 8 >= W or 16 * (t // gx) + 8 >= H)]


def view_figures(c, r, tag):
    """One view's part of check_preconditions (c: a Case or anything with its W, H, long and
    precomp; r: the oracle's result of the view): asserted, and returned as figures."""
    st = r.state()
    tiles = outside_quadrant_tiles(r, c.W, c.H)
    assert tiles, tag
    fig = dict(outside_quadrant_tiles=len(tiles))
    if c.long:
        fig["max_n_contrib"] = int(st["n_contrib"].max())
        fig["longest_list"] = int((st["ranges"][:, 1].astype(np.int64) - st["ranges"][:, 0]).max())
        assert fig["max_n_contrib"] > 1024 and fig["longest_list"] > 1024, (tag, fig)
    else:
        vis = r.radii > 0
        assert (r.radii[:40] == 0).all() and vis.sum() > 500, tag
        if not c.precomp:   # colors_precomp has no SH evaluation, hence no clamp
            fig["clamped_fraction"] = float(st["clamped"][vis].mean())
            assert fig["clamped_fraction"] >= 0.05, (tag, fig)
        fig["capped_pairs"] = capped_pairs(r, c.W, c.H)
        assert fig["capped_pairs"] >= 20, (tag, fig)
    return fig


def check_preconditions(name, ref):
    """What each scene must exercise, asserted on the oracle's state (so that a scene cannot
    silently stop reaching its branch).  Returns the measured figures."""
    c = case(name)
    out = {v: view_figures(c, r, (name, v)) for v, r in enumerate(ref.views)}
    if c.precomp:
        assert np.abs(ref.grads["cov3D"]).max() > 0 and np.abs(ref.grads["colors"]).max() > 0
    return out


def check_preprocess_preconditions(name, ref):
    """What a PP_CASES scene must give the per-Gaussian kernel's 256-row blocks, asserted on the
    oracle's state: a last block that is partial, a block with culled and visible rows side by
    side, SH colour channels clamped at 0 where SH is evaluated.  PP_EXTRA scenes, on the float
    oracle: at least 20 visible rows outside the 1.3 tan(fov) clamp, at least 20 of them with a
    means3D gradient, at least 16 visible rows of opacity <= 0.003; NEAR: exactly the rows with
    z > 0.2f of its six are kept.  Returns the measured figures."""
    c, st = case(name), ref.views[0].state()
    P = c.scene.P
    vis = st["tiles"] > 0
    mixed = [b for b in range(0, P, 256) if vis[b:b + 256].any() and not vis[b:b + 256].all()]
    fig = dict(P=P, last_block_rows=P % 256, visible=int(vis.sum()), mixed_blocks=len(mixed))
    assert 256 < P < 1000 and P % 256 != 0 and mixed and vis[P - P % 256:].any(), (name, fig)
    assert not vis[:40].any() and vis[40:256].any(), (name, fig)
    if c.colors is None:
        assert c.scene.shs.shape[1] == pp_spec(name).get("M", 16) >= (c.sh_degree + 1) ** 2, name
        fig["clamped_fraction"] = float(st["clamped"][vis].mean())
        assert fig["clamped_fraction"] >= 0.05, (name, fig)
    else:
        assert np.abs(ref.grads["colors"]).max() > 0, name
    if c.cov3D:
        assert np.abs(ref.grads["cov3D"]).max() > 0, name
    if name in PP_EXTRA:
        assert not ref.views[0].double, name      # the counts below are the float oracle's
        seen = ref.views[0].radii > 0
        fc = frustum_clamped(c.scene, c.cams[0]) & seen
        faint = seen & (c.scene.opacities.numpy().reshape(-1) <= np.float32(0.003))
        moved = fc & (ref.grads["means3D"] != 0).any(axis=1)
        fig.update(frustum_clamped=int(fc.sum()), faint_visible=int(faint.sum()), frustum_clamped_with_grad=int(moved.sum()),
                   max_clamped_means3D_grad=float(np.abs(ref.grads["means3D"][fc]).max()))
        assert fig["frustum_clamped"] >= 20 and fig["faint_visible"] >= 16, (name, fig)
        assert fig["frustum_clamped_with_grad"] >= 20, (name, fig)
        if pp_spec(name).get("near"):
            near = seen[NEAR_ROWS]
            fig["near_kept"] = int(near.sum())
            assert np.array_equal(near, NEAR_KEPT) and NEAR_KEPT.sum() == 3, (name, near)
    return fig


def frustum_clamped(scene, cam):
    """Rows whose view-space x / z or y / z lies outside 1.3 tan(fov): the clamp of computeCov2D,
    decided on the same float quotients as the oracle and the kernels."""
    m = cam.world_view_transform.numpy().astype(np.float32).reshape(-1)
    p = scene.means3D.numpy().astype(np.float32)
    t = [m[k] * p[:, 0] + m[4 + k] * p[:, 1] + m[8 + k] * p[:, 2] + m[12 + k] for k in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        txtz, tytz = t[0] / t[2], t[1] / t[2]
    limx, limy = np.float32(1.3) * np.float32(cam.tanfovx), np.float32(1.3) * np.float32(cam.tanfovy)
    return (np.abs(txtz) > limx) | (np.abs(tytz) > limy)
