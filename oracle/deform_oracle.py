"""CPU restatement of the 4D-LangSplat deformation network forward and backward (numpy, float64).

TEST INFRASTRUCTURE ONLY: imported by tests/ as the checker of the HIP deformation kernels
(4dlangsplat_amd/csrc/deform.hip); never part of the product path.

Parity: pinned on the reference module itself.  tests/golden/deform_golden.npz holds inputs,
parameters, outputs and autograd gradients of the reference `deform_network` (generated in the
build container by tests/golden/make_deform_golden.py), and tests/test_deform_oracle.py checks this
restatement against them.

Beside the float64 restatement (the default, which those pins hold) DeformOracle has, for the
per-element tests of the kernels (tests/test_deform_branches_gpu.py, tests/test_deform_check.py):
coords="float32", the kernels' own float32 cell, fraction and border-mask decisions under float64
values; train_aabb, the box's gradient grid.aabb among the parameter gradients;
forward / backward(abs_terms=True), the term scale A of every output and gradient; and
products="bf16x3", an emulation of the kernels' bf16 hi / lo matrix products.  The class docstring
describes them.

Follows (reference file:line):
  normalize_aabb                      scene/hexplane.py:19-20
  grid_sample_wrapper (bilinear, align_corners=True, padding_mode='border')   :21-46
  interpolate_ms_features (product over the 6 planes, concat over scales)     :73-106
  HexPlaneField.get_density (pts ++ t, plane list per scale)                  :160-177
  Deformation.query_time / create_net (feature_out: max(defor_depth, 1) Linear layers with ReLU
                                      between them)  scene/deformation.py:45-86
  Deformation.forward_dynamic         :103-182 -- residual heads (each can be off: no_dx / no_ds /
                                      no_dr / no_do / no_dshs), apply_rotation (quaternion product and
                                      normalisation, utils/graphics_utils.py:109-132), and the language
                                      modes: pass-through (no_dlang), lang_deform over
                                      [lang ++ poc_fre(t)] with residual (or not: no_resnet) and
                                      re-normalisation (:164-180), or the discrete centres with the
                                      discrete_coff_generator head (use_discrete_lang_f, :156-163)
  deform_network.forward_dynamic      :232-248, poc_fre :261-267 (rays_pts_emb[:, :3] == means3D;
                                      only the time embedding feeds a computed path: lang_deform)
Layouts: plane of combo (c0, c1) is [C, res[c1], res[c0]] (x along res[c0]); Linear weights are
[out, in] as torch.
"""
import itertools

import numpy as np

HEADS = (("pos_deform", 3), ("scales_deform", 3), ("rotations_deform", 4), ("opacity_deform", 1),
         ("shs_deform", 48))
COMBOS = list(itertools.combinations(range(4), 2))   # xy, xz, xt, yz, yt, zt


def plane_key(scale, ci):
    return f"grid.grids.{scale}.{ci}"


def _axis(x, n):
    """One axis of tap_of (csrc/deform_field.h): cell, fraction and the border mask 0 < r < n - 1 of
    the unclamped pixel coordinate r.  x float64: in float64; x float32: every operation a correctly
    rounded float32 one in the kernel's order, ((x + 1) * 0.5) * (n - 1), the clamp, floor and
    ix - x0 (the cell and mask decisions are then the kernel's bit for bit); fraction as float64."""
    t = x.dtype.type
    r = (x + t(1.0)) * t(0.5) * t(n - 1)
    ix = np.minimum(np.maximum(r, t(0.0)), t(n - 1))
    f0 = np.floor(ix)
    i0 = f0.astype(np.int64)
    return i0, np.minimum(i0 + 1, n - 1), (ix - f0).astype(np.float64), (r > 0) & (r < t(n - 1))


def _sample(plane, x, y):
    """Bilinear sample of plane [C, H, W] at normalised coords x, y in [-1, 1] (align_corners,
    border; x1 / y1 clamped to the last cell, where their weight is 0).  Returns values [P, C] and the
    tap description for the backward.  x, y float32: the coordinate decisions in float32 (_axis)."""
    C, H, W = plane.shape
    x0, x1, fx, mx = _axis(x, W)
    y0, y1, fy, my = _axis(y, H)
    v00, v01 = plane[:, y0, x0].T, plane[:, y0, x1].T
    v10, v11 = plane[:, y1, x0].T, plane[:, y1, x1].T
    val = (v00 * ((1 - fx) * (1 - fy))[:, None] + v01 * (fx * (1 - fy))[:, None]
           + v10 * ((1 - fx) * fy)[:, None] + v11 * (fx * fy)[:, None])
    return val, (x0, x1, y0, y1, fx, fy, v00, v01, v10, v11, mx, my, W, H)


def _scatter(gp, yy, xx, vals):
    """gp[c, yy[p], xx[p]] += vals[p, c], in the order of p."""
    C, H, W = gp.shape
    idx = (yy * W + xx)[:, None] + (np.arange(C) * (H * W))[None, :]
    gp += np.bincount(idx.ravel(), vals.ravel(), minlength=C * H * W).reshape(C, H, W)


def _bf16(x):
    """float32 -> the nearest bf16 (ties to even), as float32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)).view(np.float32)


def _split(x):
    x = np.ascontiguousarray(x, np.float32)
    hi = _bf16(x)
    return hi, _bf16(x - hi)


def _relu(x):
    return np.maximum(x, 0.0)


HEAD_NAMES = ("pos_deform", "scales_deform", "rotations_deform", "opacity_deform", "shs_deform")


class DeformConfig:
    """The switches of scene/deformation.py that change the computation (ModelHiddenParams plus the
    env vars the reference reads).  lang_mode: "pass" (no_dlang), "residual" (lang_deform),
    "noresnet" (lang_deform, env no_resnet=t) or "discrete" (env use_discrete_lang_f=t)."""

    def __init__(self, n_scales=2, depth=0, heads=(True, True, True, True, True), apply_rotation=False,
                 lang_mode="pass", lang_dim=3, centers=0, time_pe=4):
        self.n_scales, self.depth, self.heads = n_scales, depth, tuple(bool(h) for h in heads)
        self.apply_rotation, self.lang_mode, self.lang_dim = apply_rotation, lang_mode, lang_dim
        self.centers, self.time_pe = centers, time_pe

    @classmethod
    def from_golden(cls, cfg):
        """From the config dict of tests/golden/deform_variants.npz."""
        mode = "pass" if cfg["no_dlang"] else ("discrete" if cfg["discrete"] else
                                               ("noresnet" if cfg["no_resnet"] else "residual"))
        return cls(len(cfg["multires"]), cfg["depth"], tuple(not cfg[k] for k in ("no_dx", "no_ds", "no_dr", "no_do",
                                                                                   "no_dshs")),
                   cfg["apply_rotation"], mode, cfg["lang_dim"], cfg["centers"], cfg["time_pe"])


def poc_fre(x, n):
    """[x, sin(x 2^i), cos(x 2^i)] for i < n, as deformation.py:261-267 (x: [P, k])."""
    e = (x[:, :, None] * (2.0 ** np.arange(n))[None, None, :]).reshape(x.shape[0], -1)
    return np.concatenate([x, np.sin(e), np.cos(e)], axis=1)


def quat_mul(q1, q2):
    """batch_quaternion_multiply before its normalisation (utils/graphics_utils.py:121-124)."""
    w = q1[:, 0] * q2[:, 0] - q1[:, 1] * q2[:, 1] - q1[:, 2] * q2[:, 2] - q1[:, 3] * q2[:, 3]
    x = q1[:, 0] * q2[:, 1] + q1[:, 1] * q2[:, 0] + q1[:, 2] * q2[:, 3] - q1[:, 3] * q2[:, 2]
    y = q1[:, 0] * q2[:, 2] - q1[:, 1] * q2[:, 3] + q1[:, 2] * q2[:, 0] + q1[:, 3] * q2[:, 1]
    z = q1[:, 0] * q2[:, 3] + q1[:, 1] * q2[:, 2] - q1[:, 2] * q2[:, 1] + q1[:, 3] * q2[:, 0]
    return np.stack([w, x, y, z], axis=1)


def quat_mul_abs(a1, a2):
    """quat_mul on magnitudes: each component as the sum of the magnitudes of its four products."""
    i = np.array([[0, 1, 2, 3], [1, 0, 3, 2], [2, 3, 0, 1], [3, 2, 1, 0]])   # q2 index per (component, q1 index)
    return np.stack([(a1 * a2[:, i[k]]).sum(1) for k in range(4)], axis=1)


def quat_mul_bwd(q1, q2, d):
    """Gradients of sum(quat_mul(q1, q2) * d) w.r.t. q1 and q2."""
    e = np.eye(4)
    d1 = np.stack([(quat_mul(np.broadcast_to(e[k], q1.shape), q2) * d).sum(1) for k in range(4)], axis=1)
    d2 = np.stack([(quat_mul(q1, np.broadcast_to(e[k], q2.shape)) * d).sum(1) for k in range(4)], axis=1)
    return d1, d2


def normalize_bwd(v, d, eps):
    """Gradient of sum(v / (|v| + eps) * d) w.r.t. v (rows)."""
    n = np.linalg.norm(v, axis=1, keepdims=True)
    return d / (n + eps) - v * ((v * d).sum(1, keepdims=True) / (n * (n + eps) ** 2))


def _norm_abs(v, Av, n):
    """Term scale of v / n, n = |v|: the quotient's own terms and those of the norm's squares."""
    return Av / n + np.abs(v) * ((np.abs(v) * Av).sum(-1, keepdims=True) / n ** 3)


def _norm_bwd_abs(v, Ad, n, eps):
    """Term scale of normalize_bwd: both of its terms with the magnitudes of their products."""
    return Ad / (n + eps) + np.abs(v) * ((np.abs(v) * Ad).sum(-1, keepdims=True) / (n * (n + eps) ** 2))


class DeformOracle:
    """params: dict name -> array, names as in the reference Deformation module
    (grid.grids.{s}.{ci}, feature_out.{2k}.weight / .bias, {head}.1 / .3 weight / bias,
    discrete_coff_generator.1 / .3, lang_deform.1 / .3 / .5).  cfg: DeformConfig (default: the
    Neu3D structure, arguments/neu3d/default.py).

    coords: "float64" (default), or "float32": the normalised coordinates and every cell, fraction
    and border-mask decision of the plane taps in numpy float32, operation by operation as coords() /
    tap_of() / the backward's masks of csrc/deform_field.h and deform.hip (built without contraction
    and with correctly rounded division, so numpy float32 reproduces them bit for bit); the values
    stay float64.  With it a point exactly on a grid line, on a box face or past the last cell takes
    the kernel's cell and the kernel's mask, as the rasterizer's oracle shares its alpha and T.

    products: "float64" (default), or "bf16x3", an emulation of the kernels' matrix products: every
    Linear product, forward and backward, takes both operands as bf16 hi + lo, forms
    hi hi + hi lo + lo hi and accumulates in float32.  It overstates the kernels (the small heads'
    G W2 runs on the fp32 VALU) and exists so that a check's coefficient can be judged on the CPU.
    drop_lo_hi: a layer name whose products leave the lo hi term out (a test's doctored emulation).

    forward(..., abs_terms=True) returns (res, A) and backward(..., abs_terms=True) returns
    (g_in, g, A_in, A_g): beside every output offset and every input and parameter gradient its term
    scale A, the same computation with every factor replaced by its magnitude -- |weights|, |biases|,
    |upstream|, |plane taps|, the other planes' |samples|, tap differences as sums of magnitudes,
    the quaternion product / the normalisations / the discrete combination as the sums of the
    magnitudes of their products -- carried through the chain of layers (a layer's input enters with
    its own A), the ReLU and border masks kept.  A >= |value| per element; an element nothing flows
    into has A = 0.  A of an output whose head is off (it is its input) is 0; A of an input gradient
    that is the upstream itself is |upstream|.
    The box is the exception to the chain: carried through, the scale of grid.aabb -- a sum over every
    Gaussian of a coordinate gradient whose tap differences enter as sums of magnitudes -- is 1e4 to
    1e6 times the gradient and bounds nothing.  Its A is sum_p (|n| + 1) / 2 |s| sum |dv_c gx_c|
    (W - 1) / 2 over the last products of the coordinate gradient, taken on the values: the plane
    gradient dv of channel c times the tap slope gx, per plane, scale and channel, border masks kept.

    train_aabb (as DeformationField.train_aabb): the parameter gradients include grid.aabb
    (hexplane.py normalize_aabb: n = (p - a0) s - 1,
    s = 2 / (a1 - a0), so dL/da0 = sum dL/dp (n - 1) / 2 and dL/da1 = -sum dL/dp (n + 1) / 2 over the
    gradient dL/dp that reaches p through the coordinates)."""

    def __init__(self, params, aabb, n_scales=2, cfg=None, coords="float64", products="float64", drop_lo_hi=None,
                 train_aabb=False):
        assert coords in ("float64", "float32") and products in ("float64", "bf16x3")
        self.p = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
        self.aabb = np.asarray(aabb, dtype=np.float64)
        self.cfg = cfg or DeformConfig(n_scales=n_scales)
        self.n_scales = self.cfg.n_scales
        self.coords, self.products, self.drop_lo_hi, self.train_aabb = coords, products, drop_lo_hi, train_aabb

    def _mm(self, a, b, layer=None):
        """a @ b of a Linear layer (forward or backward)."""
        if self.products == "float64":
            return a @ b
        (ah, al), (bh, bl) = _split(a), _split(b)
        r = ah @ bh + ah @ bl
        if layer is None or layer != self.drop_lo_hi:
            r = r + al @ bh
        return r.astype(np.float64)

    def normalised(self, means3D, time):
        """[P, 4] normalised coordinates ++ time, in the dtype of the coords mode."""
        t = np.float32 if self.coords == "float32" else np.float64
        m, a0, a1 = means3D.astype(t), self.aabb[0].astype(t), self.aabb[1].astype(t)
        pn = (m - a0) * (t(2.0) / (a1 - a0)) - t(1.0)
        return np.concatenate([pn, time.reshape(-1, 1).astype(t)], axis=1)

    def features(self, means3D, time):
        q = self.normalised(means3D, time)
        feats, taps = [], []
        for s in range(self.n_scales):
            prod = None
            vals, tp = [], []
            for ci, (c0, c1) in enumerate(COMBOS):
                plane = self.p[plane_key(s, ci)][0]
                v, t = _sample(plane, q[:, c0], q[:, c1])
                vals.append(v)
                tp.append(t)
                prod = v if prod is None else prod * v
            feats.append(prod)
            taps.append((vals, tp))
        self._q = q.astype(np.float64)
        return np.concatenate(feats, axis=1), taps

    def _abs_samples(self, taps):
        """|samples| of every plane: the bilinear weights are non-negative, the taps enter as |tap|."""
        out = []
        for vals, tp in taps:
            av = []
            for (x0, x1, y0, y1, fx, fy, v00, v01, v10, v11, mx, my, W, H) in tp:
                av.append(np.abs(v00) * ((1 - fx) * (1 - fy))[:, None] + np.abs(v01) * (fx * (1 - fy))[:, None]
                          + np.abs(v10) * ((1 - fx) * fy)[:, None] + np.abs(v11) * (fx * fy)[:, None])
            out.append(av)
        return out

    def _lin(self, name, x):
        return self._mm(x, self.p[name + ".weight"].T, name) + self.p[name + ".bias"]

    def _lin_abs(self, name, Ax):
        return Ax @ np.abs(self.p[name + ".weight"]).T + np.abs(self.p[name + ".bias"])

    def _heads(self):
        c = self.cfg
        hs = [(n, w) for (n, w), on in zip(HEADS, c.heads) if on]
        if c.lang_mode == "discrete":
            hs.append(("discrete_coff_generator", c.centers))
        return hs

    def forward(self, means3D, scales, rotations, opacity, shs, lang, time, abs_terms=False):
        c = self.cfg
        P = means3D.shape[0]
        feat, taps = self.features(means3D, time)
        pre, acts = [], [feat]
        for k in range(max(c.depth, 1)):        # feature_out.{2k}, ReLU before the next layer / the heads
            pre.append(self._lin(f"feature_out.{2 * k}", acts[-1]))
            acts.append(_relu(pre[-1]))
        a = acts[-1]
        outs, cache = {}, {}
        for name, n in self._heads():
            z = self._lin(name + ".1", a)
            a2 = _relu(z)
            outs[name] = self._lin(name + ".3", a2)
            cache[name] = (z, a2)
        res = dict(means3D=means3D + outs["pos_deform"] if c.heads[0] else means3D.copy(),
                   scales=scales + outs["scales_deform"] if c.heads[1] else scales.copy(),
                   opacity=opacity + outs["opacity_deform"] if c.heads[3] else opacity.copy(),
                   shs=shs + outs["shs_deform"].reshape(-1, 16, 3) if c.heads[4] else shs.copy(), coff=None)
        rq = None
        if not c.heads[2]:
            res["rotations"] = rotations.copy()
        elif c.apply_rotation:
            rq = quat_mul(rotations, outs["rotations_deform"])
            res["rotations"] = rq / np.linalg.norm(rq, axis=1, keepdims=True)
        else:
            res["rotations"] = rotations + outs["rotations_deform"]
        lc = None
        if c.lang_mode == "pass":
            res["lang"] = None if lang is None else lang[:, :c.lang_dim].copy()
        elif c.lang_mode == "discrete":
            e = lang[:, :c.lang_dim * c.centers].reshape(P, c.centers, c.lang_dim)
            en = np.linalg.norm(e, axis=2, keepdims=True)
            u = e / en
            coff = outs["discrete_coff_generator"]
            m = (coff[:, :, None] * u).sum(1)
            res["lang"] = m / (np.linalg.norm(m, axis=1, keepdims=True) + 1e-9)
            res["coff"] = coff
            lc = (e, en, u, coff, m)
        else:
            x0 = np.concatenate([lang, poc_fre(time.reshape(-1, 1), c.time_pe)], axis=1)
            u0 = _relu(x0)
            z1 = self._lin("lang_deform.1", u0)
            u1 = _relu(z1)
            z2 = self._lin("lang_deform.3", u1)
            u2 = _relu(z2)
            dl = self._lin("lang_deform.5", u2)
            v = dl if c.lang_mode == "noresnet" else lang[:, :c.lang_dim] + dl
            res["lang"] = v / (np.linalg.norm(v, axis=1, keepdims=True) + 1e-9)
            lc = (x0, u0, z1, u1, z2, u2, v)
        self._cache = (feat, taps, pre[-1], a, cache, P)
        self._full = dict(pre=pre, acts=acts, rq=rq, rotations=rotations, outs=outs, lc=lc, lang=lang)
        if not abs_terms:
            return res
        # ---- term scales: the same chain on magnitudes, the ReLU masks of the values kept ----------
        Asamp = self._abs_samples(taps)
        Aacts = [np.concatenate([np.prod(av, axis=0) for av in Asamp], axis=1)]
        for k in range(max(c.depth, 1)):
            Aacts.append(self._lin_abs(f"feature_out.{2 * k}", Aacts[-1]) * (pre[k] > 0))
        Aout, Aa2 = {}, {}
        for name, n in self._heads():
            Aa2[name] = self._lin_abs(name + ".1", Aacts[-1]) * (cache[name][0] > 0)
            Aout[name] = self._lin_abs(name + ".3", Aa2[name])
        zero = lambda x: np.zeros(np.shape(x))   # noqa: E731
        A = dict(means3D=Aout["pos_deform"] if c.heads[0] else zero(means3D),
                 scales=Aout["scales_deform"] if c.heads[1] else zero(scales),
                 opacity=Aout["opacity_deform"] if c.heads[3] else zero(opacity),
                 shs=Aout["shs_deform"].reshape(-1, 16, 3) if c.heads[4] else zero(shs), coff=None)
        if not c.heads[2]:
            A["rotations"] = zero(rotations)
        elif c.apply_rotation:
            Arq = quat_mul_abs(np.abs(rotations), Aout["rotations_deform"])
            A["rotations"] = _norm_abs(rq, Arq, np.linalg.norm(rq, axis=1, keepdims=True))
        else:
            A["rotations"] = Aout["rotations_deform"]
        Alc = None
        if c.lang_mode == "pass":
            A["lang"] = None if lang is None else zero(res["lang"])
        elif c.lang_mode == "discrete":
            Acoff = Aout["discrete_coff_generator"]
            Am = (Acoff[:, :, None] * np.abs(u)).sum(1)
            A["lang"] = _norm_abs(m, Am, np.linalg.norm(m, axis=1, keepdims=True) + 1e-9)
            A["coff"] = Acoff
        else:
            Au1 = self._lin_abs("lang_deform.1", u0) * (z1 > 0)
            Au2 = self._lin_abs("lang_deform.3", Au1) * (z2 > 0)
            Av = self._lin_abs("lang_deform.5", Au2)
            if c.lang_mode != "noresnet":
                Av = Av + np.abs(lang[:, :c.lang_dim])
            A["lang"] = _norm_abs(v, Av, np.linalg.norm(v, axis=1, keepdims=True) + 1e-9)
            Alc = (Au1, Au2)
        self._abs = dict(samp=Asamp, acts=Aacts, a2=Aa2, outs=Aout, lc=Alc)
        return res, A

    def preactivations(self):
        """Every ReLU input of the last forward (for tests that avoid ReLU kinks)."""
        f = self._full
        zs = list(f["pre"]) + [z for z, _ in self._cache[4].values()]
        if self.cfg.lang_mode in ("residual", "noresnet"):
            lc = f["lc"]
            zs += [lc[0], lc[2], lc[4]]
        return zs

    def backward(self, up_means3D, up_scales, up_rotations, up_opacity, up_shs, up_lang=None, up_coff=None,
                 abs_terms=False):
        """Gradients of sum(out * up) w.r.t. inputs and parameters (after forward; with abs_terms after
        forward(abs_terms=True)): (g_in, g), and their term scales (A_in, A_g) with abs_terms."""
        c = self.cfg
        ab = abs_terms
        feat, taps, h, a, cache, P = self._cache
        f = self._full
        Z = self._abs if ab else None
        g, Ag = {}, {}
        g_in = dict(means3D=up_means3D.copy(), scales=up_scales.copy(), rotations=up_rotations.copy(),
                    opacity=up_opacity.copy(), shs=up_shs.copy())
        A_in = {k: np.abs(v) for k, v in g_in.items()}
        lang = f["lang"]
        if lang is None:   # pass-through with no language rows: nothing to differentiate
            lang = np.zeros((P, c.lang_dim))
        dlang_in = np.zeros_like(lang)
        Adlang = np.zeros_like(lang)
        ups = dict(pos_deform=up_means3D, scales_deform=up_scales, rotations_deform=up_rotations,
                   opacity_deform=up_opacity, shs_deform=up_shs.reshape(P, 48))
        Aups = {k: np.abs(v) for k, v in ups.items()}
        if c.heads[2] and c.apply_rotation:
            dq = normalize_bwd(f["rq"], up_rotations, 0.0)
            q1, q2 = f["rotations"], f["outs"]["rotations_deform"]
            g_in["rotations"], ups["rotations_deform"] = quat_mul_bwd(q1, q2, dq)
            if ab:
                Adq = _norm_bwd_abs(f["rq"], np.abs(up_rotations), np.linalg.norm(f["rq"], axis=1, keepdims=True), 0.0)
                e = np.eye(4)
                A_in["rotations"] = np.stack([(quat_mul_abs(np.broadcast_to(e[k], q1.shape), Z["outs"]["rotations_deform"])
                                               * Adq).sum(1) for k in range(4)], axis=1)
                Aups["rotations_deform"] = np.stack([(quat_mul_abs(np.abs(q1), np.broadcast_to(e[k], q2.shape)) * Adq).sum(1)
                                                     for k in range(4)], axis=1)
        up_lang = np.zeros((P, c.lang_dim)) if up_lang is None else up_lang
        if c.lang_mode == "pass":
            dlang_in[:, :c.lang_dim] += up_lang
            Adlang[:, :c.lang_dim] += np.abs(up_lang)
        elif c.lang_mode == "discrete":
            e, en, u, coff, m = f["lc"]
            dm = normalize_bwd(m, up_lang, 1e-9)
            dcoff = (u * dm[:, None, :]).sum(2) + (0.0 if up_coff is None else up_coff)
            du = coff[:, :, None] * dm[:, None, :]
            de = (du - u * (u * du).sum(2, keepdims=True)) / en
            dlang_in[:, :c.lang_dim * c.centers] += de.reshape(P, -1)
            ups["discrete_coff_generator"] = dcoff
            if ab:
                Adm = _norm_bwd_abs(m, np.abs(up_lang), np.linalg.norm(m, axis=1, keepdims=True), 1e-9)
                Aups["discrete_coff_generator"] = (np.abs(u) * Adm[:, None, :]).sum(2) + (0.0 if up_coff is None
                                                                                            else np.abs(up_coff))
                Adu = Z["outs"]["discrete_coff_generator"][:, :, None] * Adm[:, None, :]
                Ade = (Adu + np.abs(u) * (np.abs(u) * Adu).sum(2, keepdims=True)) / en
                Adlang[:, :c.lang_dim * c.centers] += Ade.reshape(P, -1)
        else:
            x0, u0, z1, u1, z2, u2, v = f["lc"]
            dv = normalize_bwd(v, up_lang, 1e-9)
            if c.lang_mode == "residual":
                dlang_in[:, :c.lang_dim] += dv
            g["lang_deform.5.weight"] = self._mm(dv.T, u2, "lang_deform.5")
            g["lang_deform.5.bias"] = dv.sum(0)
            dz2 = self._mm(dv, self.p["lang_deform.5.weight"], "lang_deform.5") * (z2 > 0)
            g["lang_deform.3.weight"] = self._mm(dz2.T, u1, "lang_deform.3")
            g["lang_deform.3.bias"] = dz2.sum(0)
            dz1 = self._mm(dz2, self.p["lang_deform.3.weight"], "lang_deform.3") * (z1 > 0)
            g["lang_deform.1.weight"] = self._mm(dz1.T, u0, "lang_deform.1")
            g["lang_deform.1.bias"] = dz1.sum(0)
            dx0 = self._mm(dz1, self.p["lang_deform.1.weight"], "lang_deform.1") * (x0 > 0)
            dlang_in += dx0[:, :lang.shape[1]]
            if ab:
                Au1, Au2 = Z["lc"]
                Adv = _norm_bwd_abs(v, np.abs(up_lang), np.linalg.norm(v, axis=1, keepdims=True), 1e-9)
                if c.lang_mode == "residual":
                    Adlang[:, :c.lang_dim] += Adv
                Ag["lang_deform.5.weight"], Ag["lang_deform.5.bias"] = Adv.T @ Au2, Adv.sum(0)
                Adz2 = (Adv @ np.abs(self.p["lang_deform.5.weight"])) * (z2 > 0)
                Ag["lang_deform.3.weight"], Ag["lang_deform.3.bias"] = Adz2.T @ Au1, Adz2.sum(0)
                Adz1 = (Adz2 @ np.abs(self.p["lang_deform.3.weight"])) * (z1 > 0)
                Ag["lang_deform.1.weight"], Ag["lang_deform.1.bias"] = Adz1.T @ u0, Adz1.sum(0)
                Adlang += ((Adz1 @ np.abs(self.p["lang_deform.1.weight"])) * (x0 > 0))[:, :lang.shape[1]]
        g_in["lang"], A_in["lang"] = dlang_in, Adlang
        da = np.zeros_like(a)
        Ada = np.zeros_like(a)
        for name, n in self._heads():
            z, a2 = cache[name]
            u_ = ups[name]
            g[name + ".3.weight"] = self._mm(u_.T, a2, name + ".3")
            g[name + ".3.bias"] = u_.sum(0)
            dz = self._mm(u_, self.p[name + ".3.weight"], name + ".3") * (z > 0)
            g[name + ".1.weight"] = self._mm(dz.T, a, name + ".1")
            g[name + ".1.bias"] = dz.sum(0)
            da += self._mm(dz, self.p[name + ".1.weight"], name + ".1")
            if ab:
                Au = Aups[name]
                Ag[name + ".3.weight"], Ag[name + ".3.bias"] = Au.T @ Z["a2"][name], Au.sum(0)
                Adz = (Au @ np.abs(self.p[name + ".3.weight"])) * (z > 0)
                Ag[name + ".1.weight"], Ag[name + ".1.bias"] = Adz.T @ Z["acts"][-1], Adz.sum(0)
                Ada += Adz @ np.abs(self.p[name + ".1.weight"])
        pre, acts = f["pre"], f["acts"]
        for k in reversed(range(len(pre))):
            name = f"feature_out.{2 * k}"
            dh = da * (pre[k] > 0)
            g[name + ".weight"] = self._mm(dh.T, acts[k], name)
            g[name + ".bias"] = dh.sum(0)
            da = self._mm(dh, self.p[name + ".weight"], name)
            if ab:
                Adh = Ada * (pre[k] > 0)
                Ag[name + ".weight"], Ag[name + ".bias"] = Adh.T @ Z["acts"][k], Adh.sum(0)
                Ada = Adh @ np.abs(self.p[name + ".weight"])
        dfeat, Adfeat = da, Ada
        dq, Adq = np.zeros((P, 4)), np.zeros((P, 4))
        Ldq = np.zeros((P, 4))    # the coordinate gradient's last products |dv gx|, on the values (the box's scale)
        nc = feat.shape[1] // self.n_scales
        for s in range(self.n_scales):
            vals, tp = taps[s]
            df = dfeat[:, s * nc:(s + 1) * nc]
            for ci, (c0, c1) in enumerate(COMBOS):
                others = np.ones_like(df)
                for cj in range(len(COMBOS)):
                    if cj != ci:
                        others = others * vals[cj]
                dv = df * others                                       # [P, C]
                x0_, x1_, y0_, y1_, fx, fy, v00, v01, v10, v11, mx, my, W, H = tp[ci]
                key = plane_key(s, ci)
                gp = g.setdefault(key, np.zeros_like(self.p[key]))[0]
                wts = ((y0_, x0_, (1 - fx) * (1 - fy)), (y0_, x1_, fx * (1 - fy)), (y1_, x0_, (1 - fx) * fy),
                       (y1_, x1_, fx * fy))
                for (yy, xx, w) in wts:
                    _scatter(gp, yy, xx, dv * w[:, None])
                dix = (dv * ((v01 - v00) * (1 - fy)[:, None] + (v11 - v10) * fy[:, None])).sum(1)
                diy = (dv * ((v10 - v00) * (1 - fx)[:, None] + (v11 - v01) * fx[:, None])).sum(1)
                # border padding: no gradient through a clipped coordinate (clip at <= 0, >= size-1)
                dq[:, c0] += dix * 0.5 * (W - 1) * mx
                dq[:, c1] += diy * 0.5 * (H - 1) * my
                if ab:
                    gx = (v01 - v00) * (1 - fy)[:, None] + (v11 - v10) * fy[:, None]
                    gy = (v10 - v00) * (1 - fx)[:, None] + (v11 - v01) * fx[:, None]
                    Ldq[:, c0] += np.abs(dv * gx).sum(1) * 0.5 * (W - 1) * mx
                    Ldq[:, c1] += np.abs(dv * gy).sum(1) * 0.5 * (H - 1) * my
                    Av = Z["samp"][s]
                    Adv = Adfeat[:, s * nc:(s + 1) * nc] * np.prod([Av[cj] for cj in range(len(COMBOS)) if cj != ci],
                                                                   axis=0)
                    Agp = Ag.setdefault(key, np.zeros_like(self.p[key]))[0]
                    for (yy, xx, w) in wts:
                        _scatter(Agp, yy, xx, Adv * w[:, None])
                    b00, b01, b10, b11 = np.abs(v00), np.abs(v01), np.abs(v10), np.abs(v11)
                    Adq[:, c0] += (Adv * ((b01 + b00) * (1 - fy)[:, None] + (b11 + b10) * fy[:, None])).sum(1) \
                        * 0.5 * (W - 1) * mx
                    Adq[:, c1] += (Adv * ((b10 + b00) * (1 - fx)[:, None] + (b11 + b01) * fx[:, None])).sum(1) \
                        * 0.5 * (H - 1) * my
        a0, a1 = self.aabb[0], self.aabb[1]
        gq = dq[:, :3] * (2.0 / (a1 - a0))
        g_in["means3D"] = g_in["means3D"] + gq
        n = self._q[:, :3]
        if self.train_aabb:
            g["grid.aabb"] = np.stack([(0.5 * gq * (n - 1.0)).sum(0), (-0.5 * gq * (n + 1.0)).sum(0)])
        if not ab:
            return g_in, g
        Agq = Adq[:, :3] * np.abs(2.0 / (a1 - a0))
        A_in["means3D"] = A_in["means3D"] + Agq
        if self.train_aabb:
            Ag["grid.aabb"] = np.stack([(0.5 * Ldq[:, :3] * np.abs(2.0 / (a1 - a0)) * (np.abs(n) + 1.0)).sum(0)] * 2)
        return g_in, g, A_in, Ag
