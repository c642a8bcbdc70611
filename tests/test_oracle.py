"""CPU tests of the oracle itself: pinned against the reference's own Python (golden vectors),
known-answer cases for the rasterizer constants, and fp64 finite differences for the backward.

The rasterizer core has no reference fixture (the CUDA source is absent: SURVEY.md 8c), so the
compositing rules are pinned by analytic known answers instead: PARITY UNPINNED vs CUDA.
"""
import math
import os

import numpy as np
import pytest

import oracle
import synthetic
from helpers import axis_camera, oracle_settings, small_case


# ---- golden vectors from the reference ---------------------------------------------------------
def test_sh_matches_reference_eval_sh(golden_dir):
    d = np.load(os.path.join(golden_dir, "sh_golden.npz"))
    for deg in range(4):
        rgb, clamped = oracle.sh_colors(deg, d[f"sh_{deg}"], d[f"pos_{deg}"], d[f"campos_{deg}"])
        np.testing.assert_allclose(rgb, d[f"rgb_{deg}"], rtol=0, atol=1e-6)
        assert ((d[f"rgb_{deg}"] == 0) >= clamped.astype(bool)).all()


def test_camera_matrices_match_reference(golden_dir):
    d = np.load(os.path.join(golden_dir, "cameras.npz"))
    for i in range(3):
        W, H = (int(v) for v in d[f"size_{i}"])
        fx, fy = d[f"fov_{i}"]
        cam = synthetic.make_camera(d[f"R_{i}"], d[f"T_{i}"], float(fx), float(fy), W, H)
        np.testing.assert_array_equal(cam.world_view_transform.numpy(), d[f"view_{i}"])
        np.testing.assert_array_equal(cam.projection_matrix.numpy(), d[f"proj_{i}"])
        np.testing.assert_allclose(cam.full_proj_transform.numpy(), d[f"full_{i}"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(cam.camera_center.numpy(), d[f"center_{i}"], rtol=0, atol=1e-6)


def test_cov3d_matches_reference(golden_dir):
    d = np.load(os.path.join(golden_dir, "cov3d.npz"))
    cov = oracle.cov3d(d["scales"], d["rotations"], float(d["mod"]))
    np.testing.assert_allclose(cov, d["cov"], rtol=1e-5, atol=2e-8)  # cancellation in tiny off-diagonals


# ---- known answers -----------------------------------------------------------------------------
def _one(cam, means, opac, colors, scales, bg=(0.2, 0.3, 0.4), lang=None):
    s = oracle_settings(cam, bg=bg, sh_degree=0, include_feature=lang is not None)
    P = len(means)
    rots = np.tile(np.array([1.0, 0, 0, 0], np.float32), (P, 1))
    return oracle.forward(s, means, opac, colors_precomp=colors, scales=scales, rotations=rots, lang=lang)


def test_single_gaussian_at_pixel_centre():
    cam = axis_camera()                       # W = H = 33: the optical axis lands on pixel (16, 16)
    o, c, bg = 0.6, np.array([0.9, 0.5, 0.1]), np.array([0.2, 0.3, 0.4])
    lang = np.array([[0.6, -0.8, 0.0]], np.float32)
    r = _one(cam, [[0, 0, 3.0]], [o], [c], [[0.05, 0.05, 0.05]], bg=bg, lang=lang)
    st = r.state()
    assert r.radii[0] > 0
    np.testing.assert_allclose(st["xy"][0], [16.0, 16.0], atol=1e-5)
    np.testing.assert_allclose(r.color[:, 16, 16], o * c + (1 - o) * bg, rtol=1e-6)
    np.testing.assert_allclose(st["final_T"][16, 16], 1 - o, rtol=1e-6)
    np.testing.assert_allclose(r.lang[:, 16, 16], o * lang[0], rtol=1e-6)   # no background term
    np.testing.assert_allclose(r.depth[0, 16, 16], o * 3.0, rtol=1e-6)
    assert st["n_contrib"][16, 16] == 1


def test_two_gaussians_front_to_back():
    cam = axis_camera()
    # the nearer one (z = 2) has index 1: compositing must follow depth, not index
    cols = np.array([[1.0, 0, 0], [0, 1.0, 0]], np.float32)
    r = _one(cam, [[0, 0, 4.0], [0, 0, 2.0]], [0.5, 0.5], cols, [[0.05] * 3] * 2, bg=(0, 0, 0))
    np.testing.assert_allclose(r.color[:, 16, 16], [0.25, 0.5, 0.0], rtol=1e-6)
    st = r.state()
    t = 1 * 3 + 1                              # tile of pixel (16, 16); 3 tiles per row at W = 33
    lo, hi = st["ranges"][t]
    assert list(st["point_list"][lo:hi]) == [1, 0]


def test_alpha_cutoffs_and_clamp():
    cam = axis_camera()
    # opacity below 1/255 -> skipped entirely
    r = _one(cam, [[0, 0, 3.0]], [1.0 / 256], [[1, 1, 1]], [[0.05] * 3], bg=(0, 0, 0))
    assert r.color[:, 16, 16].max() == 0 and r.state()["n_contrib"][16, 16] == 0
    # opacity 1 -> alpha clamped at 0.99
    r = _one(cam, [[0, 0, 3.0]], [1.0], [[1, 1, 1]], [[0.05] * 3], bg=(0, 0, 0))
    np.testing.assert_allclose(r.color[:, 16, 16], 0.99, rtol=1e-6)
    np.testing.assert_allclose(r.state()["final_T"][16, 16], 0.01, rtol=1e-5)
    # three 0.99 layers: T 1 -> 0.01 -> 1e-4 (>= 1e-4 keeps going? 0.01*0.01 = 1e-4 exactly is not < 1e-4)
    # -> third would give 1e-6 < 1e-4: stops before it, and it is not a contributor
    means = [[0, 0, 2.0], [0, 0, 3.0], [0, 0, 4.0]]
    r = _one(cam, means, [1.0] * 3, [[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0.05] * 3] * 3, bg=(0, 0, 0))
    st = r.state()
    T2 = np.float32(np.float32(0.01) * np.float32(1 - np.float32(0.99)))
    if T2 < np.float32(1e-4):
        assert st["n_contrib"][16, 16] == 1
    else:
        assert st["n_contrib"][16, 16] == 2
    assert r.color[2, 16, 16] == 0.0


def test_near_plane_cull():
    cam = axis_camera()
    r = _one(cam, [[0, 0, 0.19], [0, 0, 0.21]], [0.5, 0.5], [[1, 1, 1]] * 2, [[0.001] * 3] * 2)
    assert r.radii[0] == 0 and r.radii[1] > 0
    assert list(oracle.mark_visible([[0, 0, 0.19], [0, 0, 0.21]], cam.world_view_transform.numpy())) == [False, True]


def test_precomputed_paths_agree():
    sc, cam = small_case(P=600, W=64, H=48, C=4)
    s = oracle_settings(cam)
    P = sc.P
    a = oracle.forward(s, sc.means3D, sc.opacities, shs=sc.shs, lang=sc.lang, scales=sc.scales, rotations=sc.rotations)
    cov = oracle.cov3d(sc.scales.numpy(), sc.rotations.numpy())
    b = oracle.forward(s, sc.means3D, sc.opacities, shs=sc.shs, lang=sc.lang, cov3D_precomp=cov)
    np.testing.assert_array_equal(a.radii, b.radii)
    np.testing.assert_allclose(a.color, b.color, atol=1e-5)
    # colors_precomp = the SH colour of the same (deformed) means: identical image
    cp = a.state()["rgb"]
    c = oracle.forward(s, sc.means3D, sc.opacities, colors_precomp=cp, lang=sc.lang, scales=sc.scales,
                       rotations=sc.rotations)
    np.testing.assert_array_equal(a.color, c.color)
    assert P == a.P


# ---- finite differences (fp64 oracle) ----------------------------------------------------------
def _fd_case(seed=3):
    rng = np.random.default_rng(seed)
    P, W, H, C = 24, 40, 32, 4
    cam = synthetic.origin_camera(W, H, 0.5)
    z = rng.uniform(2.0, 4.0, P)
    means = np.stack([rng.uniform(-0.6, 0.6, P) * z * 0.5, rng.uniform(-0.6, 0.6, P) * z * 0.4, z], 1)
    scales = np.exp(rng.normal(-2.6, 0.25, (P, 3)))
    q = rng.normal(size=(P, 4))
    rots = q / np.linalg.norm(q, axis=1, keepdims=True)
    opac = rng.uniform(0.1, 0.6, P)
    shs = rng.normal(0, 0.3, (P, 16, 3))
    shs[:, 0] += 1.2                       # keep colours away from the clamp at 0
    lang = rng.normal(size=(P, C))
    return cam, dict(means3D=means, scales=scales, rotations=rots, opacities=opac, shs=shs, lang=lang)


def _loss(s, inp, wts, double=True):
    r = oracle.forward(s, inp["means3D"], inp["opacities"], shs=inp["shs"], lang=inp["lang"], scales=inp["scales"],
                       rotations=inp["rotations"], double=double, nthreads=1)
    L = (r.color * wts[0]).sum() + (r.lang * wts[1]).sum() + (r.depth[0] * wts[2]).sum()
    return L, r


@pytest.mark.parametrize("seed", [3, 11])
def test_backward_matches_finite_differences(seed):
    cam, inp = _fd_case(seed)
    s = oracle_settings(cam, bg=(0.3, 0.6, 0.9))
    H, W, C = cam.image_height, cam.image_width, inp["lang"].shape[1]
    rng = np.random.default_rng(100 + seed)
    wts = (rng.normal(size=(3, H, W)), rng.normal(size=(C, H, W)), rng.normal(size=(H, W)))
    L0, r = _loss(s, inp, wts)
    g = r.backward(wts[0], wts[1], wts[2], nthreads=1)
    # no pixel may sit on a discontinuity (alpha clamp / cut-offs) for the FD to be meaningful
    eps = 1e-6
    checks = {"means3D": "means3D", "scales": "scales", "rotations": "rotations", "opacities": "opacity",
              "shs": "sh", "lang": "lang"}
    vis = np.nonzero(r.radii > 0)[0]
    assert len(vis) > 10
    for name, gname in checks.items():
        base = inp[name]
        ana = g[gname].reshape(base.shape[0], -1)
        idx = [(i, j) for i in vis[:8] for j in range(min(ana.shape[1], 4 if name != "shs" else 48))]
        for (i, j) in idx:
            pert = {k: v.copy() for k, v in inp.items()}
            flat = pert[name].reshape(base.shape[0], -1)
            flat[i, j] += eps
            Lp, rp = _loss(s, pert, wts)
            flat[i, j] -= 2 * eps
            Lm, rm = _loss(s, pert, wts)
            if not (np.array_equal(rp.radii, r.radii) and np.array_equal(rm.radii, r.radii)):
                continue
            fd = (Lp - Lm) / (2 * eps)
            scale = max(1.0, abs(fd))
            assert abs(fd - ana[i, j]) <= 2e-4 * scale, (name, i, j, fd, ana[i, j])


def _fd_branch(settings_kw, precomp=False, seed=3):
    """test_backward_matches_finite_differences (same _fd_case, eps and tolerance) on the oracle's
    other branches: settings_kw goes to oracle_settings; precomp renders from cov3D_precomp and
    colors_precomp and checks their gradients instead of those of scales, rotations and SH."""
    cam, inp = _fd_case(seed)
    if precomp:
        inp["cov3D"] = oracle.cov3d(inp.pop("scales"), inp.pop("rotations"), double=True)
        inp["colors"] = np.random.default_rng(seed).uniform(0.2, 1.0, (len(inp["cov3D"]), 3))
        del inp["shs"]
    s = oracle_settings(cam, bg=(0.3, 0.6, 0.9), **settings_kw)
    H, W, C = cam.image_height, cam.image_width, inp["lang"].shape[1]
    rng = np.random.default_rng(100 + seed)
    wts = (rng.normal(size=(3, H, W)), rng.normal(size=(C, H, W)), rng.normal(size=(H, W)))

    def loss(x):
        kw = dict(cov3D_precomp=x["cov3D"], colors_precomp=x["colors"]) if precomp else dict(
            shs=x["shs"], scales=x["scales"], rotations=x["rotations"])
        r = oracle.forward(s, x["means3D"], x["opacities"], lang=x["lang"], double=True, nthreads=1, **kw)
        return (r.color * wts[0]).sum() + (r.lang * wts[1]).sum() + (r.depth[0] * wts[2]).sum(), r

    L0, r = loss(inp)
    g = r.backward(wts[0], wts[1], wts[2], nthreads=1)
    eps = 1e-6
    checks = {"means3D": "means3D", "opacities": "opacity", "lang": "lang"}
    checks.update({"cov3D": "cov3D", "colors": "colors"} if precomp else
                  {"scales": "scales", "rotations": "rotations", "shs": "sh"})
    vis = np.nonzero(r.radii > 0)[0]
    assert len(vis) > 10
    checked = {name: 0 for name in checks}
    for name, gname in checks.items():
        base = inp[name]
        ana = g[gname].reshape(base.shape[0], -1)
        width = {"shs": 48, "cov3D": 6}.get(name, 4)
        for i in vis[:8]:
            for j in range(min(ana.shape[1], width)):
                pert = {k: v.copy() for k, v in inp.items()}
                flat = pert[name].reshape(base.shape[0], -1)
                flat[i, j] += eps
                Lp, rp = loss(pert)
                flat[i, j] -= 2 * eps
                Lm, rm = loss(pert)
                if not (np.array_equal(rp.radii, r.radii) and np.array_equal(rm.radii, r.radii)):
                    continue
                fd = (Lp - Lm) / (2 * eps)
                assert abs(fd - ana[i, j]) <= 2e-4 * max(1.0, abs(fd)), (name, i, j, fd, ana[i, j])
                checked[name] += ana[i, j] != 0
    assert all(n > 0 for n in checked.values()), checked   # every field had a non-zero gradient checked


@pytest.mark.parametrize("scale_modifier", [0.7, 1.6])
def test_backward_fd_scale_modifier(scale_modifier):
    """scale_modifier enters cov3D and dL/dscale; no other test passes anything but 1."""
    _fd_branch(dict(scale_modifier=scale_modifier))


@pytest.mark.parametrize("sh_degree", [0, 1, 2])
def test_backward_fd_sh_degree(sh_degree):
    _fd_branch(dict(sh_degree=sh_degree))


def test_backward_fd_precomputed():
    """cov3D_precomp + colors_precomp: dL/dcov3D and dL/dcolors against finite differences."""
    _fd_branch({}, precomp=True)
