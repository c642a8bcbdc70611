"""Every branch of the backward compositor against the oracle, element by element.

The compositor backward is five instantiations of the wave kernel's (render_bwd_wave.hip: generic,
C32, C32 + pre-split operands, no language) and the per-tile kernel (render_bwd.hip) at pads 0, 4,
8, 16, 32 and 64 in deterministic mode, pad 64 also with atomics; launch_render_bwd,
launch_render_bwd_wave_views and lsr_backward_composite_views choose.  Each case below (scenes:
bwd_cases) runs the default (atomic) and the deterministic backward on a ragged 83 x 61 image --
quadrants wholly outside it, partial ones, a tenth of the colour channels clamped, alphas at the
0.99 cap -- or on the long-replay 35 x 19 one:

    case  C        settings                    atomic kernel               deterministic kernel
    A     0        sh_degree 0                 wave, no language           per-tile pad 0
    B     5        sh_degree 3                 wave, generic               per-tile pad 8
    C     1        sh_degree 2                 wave, generic               per-tile pad 4
    D     16       scale_modifier 0.7          wave, generic               per-tile pad 16
    E     17       scale_modifier 1.6, deg 1   wave, generic               per-tile pad 32
    F     32       sh_degree 3                 wave, C32; C32 + pre-split  per-tile pad 32
    G     48       sh_degree 3                 per-tile pad 64, atomic     per-tile pad 64
    H     64       scale_modifier 0.7, deg 1   per-tile pad 64, atomic     per-tile pad 64
    P     8        cov3D + colors precomputed  wave, generic               per-tile pad 8
    L7    7        long replay (n_contrib up   wave, generic               per-tile pad 8
    L32   32         to 4098), 35 x 19         wave, C32                   per-tile pad 32
    V16   16       2 views, backward_views     wave, generic (2 views)     per view, accumulated
    V64   64       2 views, backward_views     per-tile pad 64 per view    per view, accumulated

Asserted per case: both modes pass lsr_testutil.grad_check against the float oracle (per element
|native - ref| <= 1e-4 |ref| + 1e-4 A for language, opacity and means2D, A from the oracle's
abs_terms; grad_err <= 1e-4 for every field); the deterministic gradients repeat bit for bit; atomic
against deterministic per element within 1e-4 |det| + 1e-5 max|field| for the fields derived
through the preprocess backward; the images within 1e-4 (RGB) and 1e-3 (language) and per pixel
through lsr_testutil.image_check (tests/test_forward_branches_gpu.py); equal radii; and
the scene's preconditions on the oracle's state (bwd_cases.check_preconditions).

Measured on an MI355X, against the float oracle (recorded, not used to set any bound; the last
columns are the float oracle against the double one on the same scene, tests/test_backward_check.py:
it rounds the projection as well, which the kernels share with the float oracle bit for bit).  The
atomic wave kernel's sums go through bf16 hi/lo products on the matrix cores (~2^-17 per product);
the per-tile kernel sums in fp32, so cases G, H and V64 sit with the deterministic mode.

    err / A             atomic                   deterministic            float vs double oracle
    case      language opacity means2D   language opacity means2D   language opacity means2D
    A            -    5.1e-06 3.7e-06       -    2.2e-07 2.1e-07       -    1.6e-05 1.6e-05
    B         1.3e-05 3.6e-06 4.3e-06    4.0e-07 1.7e-07 1.9e-07    3.3e-05 1.2e-05 1.5e-05
    C         1.5e-05 4.4e-06 6.5e-06    3.4e-07 2.7e-07 2.4e-07    5.8e-05 3.5e-05 5.5e-05
    D         1.5e-05 3.7e-06 5.0e-06    3.6e-07 1.8e-07 2.6e-07    3.3e-05 2.2e-05 2.0e-05
    E         1.6e-05 2.7e-06 2.3e-06    4.4e-07 1.9e-07 1.7e-07    4.0e-05 1.2e-05 9.3e-06
    F         1.6e-05 3.7e-06 2.8e-06    4.8e-07 2.2e-07 2.9e-07    3.5e-05 1.2e-05 2.5e-05
    F C32+PRE 1.6e-05 3.7e-06 2.8e-06       -       -       -       3.5e-05 1.2e-05 2.5e-05
    G         4.9e-07 2.2e-07 2.5e-07    4.9e-07 2.2e-07 2.5e-07    3.3e-05 1.9e-05 1.6e-05
    H         4.0e-07 4.1e-07 2.8e-07    4.0e-07 3.4e-07 2.8e-07    6.6e-05 2.0e-05 4.6e-05
    P         1.4e-05 3.9e-06 3.8e-06    4.8e-07 1.7e-07 2.2e-07    3.4e-05 1.2e-05 1.2e-05
    L7        1.9e-05 3.7e-06 1.6e-05    1.7e-06 4.0e-07 4.2e-07    1.1e-05 6.4e-06 1.2e-05
    L32       2.3e-05 3.2e-06 3.9e-06    2.0e-06 4.4e-07 4.9e-07    1.2e-05 5.9e-06 1.0e-05
    V16       1.4e-05 3.7e-06 3.4e-06    4.3e-07 2.4e-07 2.4e-07    3.2e-05 6.9e-06 2.1e-05
    V64       4.1e-07 3.3e-07 2.3e-07    4.1e-07 3.3e-07 2.3e-07    2.3e-05 7.5e-06 9.2e-06

    err / max|field|, the larger of the two modes (float vs double oracle in brackets)
    case      means3D           scales            rotations         sh                cov3D             colors
    A         3.6e-06 (8.5e-06) 1.2e-05 (8.8e-06) 1.3e-06 (1.5e-06) 3.4e-06 (7.0e-07) -                 3.4e-06 (7.3e-07)
    B         4.5e-06 (6.6e-06) 6.2e-06 (2.2e-06) 5.9e-06 (1.2e-06) 2.6e-06 (7.4e-07) -                 3.1e-06 (7.6e-07)
    C         4.2e-06 (5.9e-06) 6.8e-06 (2.4e-06) 3.7e-06 (1.2e-06) 2.3e-06 (9.4e-07) -                 2.3e-06 (1.1e-06)
    D         3.9e-06 (6.0e-06) 7.4e-06 (3.5e-06) 1.8e-06 (9.4e-07) 5.6e-06 (5.1e-07) -                 7.3e-06 (7.2e-07)
    E         5.6e-06 (3.3e-06) 3.2e-06 (1.9e-06) 4.0e-06 (2.8e-06) 2.7e-06 (9.5e-07) -                 2.0e-06 (1.8e-06)
    F         3.9e-06 (5.9e-06) 1.1e-05 (1.2e-05) 4.8e-06 (3.0e-06) 2.3e-06 (6.4e-07) -                 2.4e-06 (6.6e-07)
    F C32+PRE 3.9e-06 (5.9e-06) 1.1e-05 (1.2e-05) 4.8e-06 (3.0e-06) 2.3e-06 (6.4e-07) -                 2.4e-06 (6.6e-07)
    G         6.3e-07 (3.9e-06) 2.6e-06 (4.7e-06) 1.0e-06 (7.2e-06) 4.8e-07 (9.6e-07) -                 6.2e-07 (1.2e-06)
    H         8.3e-07 (1.0e-05) 7.1e-06 (3.4e-06) 3.4e-06 (5.2e-06) 8.8e-07 (8.6e-07) -                 9.6e-07 (1.1e-06)
    P         1.8e-06 (4.4e-06) -                 -                 -                 5.2e-06 (5.2e-06) 2.7e-06 (1.4e-06)
    L7        4.5e-06 (8.8e-07) 4.4e-06 (1.0e-06) 2.2e-06 (4.3e-07) 3.3e-06 (3.9e-07) -                 3.8e-06 (4.8e-07)
    L32       3.6e-06 (8.2e-07) 3.3e-06 (1.0e-06) 2.9e-06 (8.6e-07) 4.8e-06 (5.9e-07) -                 4.6e-06 (5.0e-07)
    V16       4.3e-06 (3.1e-06) 3.5e-06 (2.2e-06) 1.6e-06 (4.3e-07) 2.5e-06 (1.1e-06) -                 2.6e-06 (1.1e-06)
    V64       6.4e-07 (4.5e-06) 5.3e-06 (2.8e-06) 9.0e-06 (6.0e-06) 1.1e-06 (5.2e-07) -                 9.6e-07 (5.4e-07)
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # CPU container: the driver only runs these on the MI355X box
    pytest.skip("needs a GPU", allow_module_level=True)

import diff_gaussian_rasterization as dgr  # noqa: E402
import bwd_cases  # noqa: E402
import fwd_cases  # noqa: E402
from lsr_testutil import grad_check, image_check, oracle_keyed, raster_settings, run_native  # noqa: E402

RGB_TOL, LANG_TOL = 1e-4, 1e-3
DERIVED = ("means3D", "scales", "rotations", "sh", "cov3D", "colors")


def _dev(x):
    return None if x is None else torch.tensor(x, device="cuda")


def _expected_fields(c):
    f = {"means3D", "means2D", "colors", "opacity"}
    f |= {"cov3D"} if c.precomp else {"scales", "rotations", "sh"}
    return f | ({"lang"} if c.C else set())


def _forward(c, cam):
    """One view through run_native with the case's settings."""
    return run_native(c.scene, cam, **c.run_kw())


def _check_forward(c, nat, ref_view, view=0):
    color, lang, radii, depth, st = nat
    np.testing.assert_array_equal(radii.cpu().numpy(), ref_view.radii)
    assert np.abs(color.cpu().numpy() - ref_view.color).max() <= RGB_TOL
    if c.C:
        assert np.abs(lang.cpu().numpy() - ref_view.lang).max() <= LANG_TOL
    # and per pixel, with the exact state checks (tests/test_forward_branches_gpu.py)
    bad, stats = image_check((color, lang, depth, st), ref_view, fwd_cases.lang_scale(c.name)[view])
    assert not bad, (c.name, view, bad, stats)


def _check_grads(c, ref, atomic, dets, label):
    """atomic: one backward's dict; dets: the deterministic backward's, run twice."""
    for k, v in dets[0].items():
        assert (v is None) == (dets[1][k] is None) and (v is None or torch.equal(v, dets[1][k])), (label, k)
    ga, gd = oracle_keyed(atomic), oracle_keyed(dets[0])
    assert set(ga) == _expected_fields(c) == set(gd), (label, sorted(ga), sorted(gd))
    report = {}
    for mode, g in (("atomic", ga), ("deterministic", gd)):
        bad, stats = grad_check(g, ref.grads, ref.abs)
        report[mode] = stats
        print(label, mode, {k: {n: float(f"{x:.2e}") for n, x in s.items()} for k, s in stats.items()})
        assert not bad, (label, mode, bad, stats)
    derived = {}
    for k in DERIVED:
        if k in ga:
            err, fmax = np.abs(ga[k] - gd[k]), np.abs(gd[k]).max()
            derived[k] = float(err.max() / max(fmax, 1e-30))
            assert (err <= 1e-4 * np.abs(gd[k]) + 1e-5 * fmax).all(), (label, k, derived[k])
    print(label, "atomic vs deterministic / max|field|", {k: float(f"{x:.2e}") for k, x in derived.items()})
    return report


def _single_view(name):
    c, ref = bwd_cases.case(name), bwd_cases.reference(name)
    bwd_cases.check_preconditions(name, ref)
    nat = _forward(c, c.cams[0])
    _check_forward(c, nat, ref.views[0])
    gc, gl, gd = _dev(c.gcol[0]), _dev(c.glang[0]), _dev(c.gdep[0])
    atomic = dgr.backward_native(nat[4], gc, gl, gd)
    dets = [dgr.backward_native(nat[4], gc, gl, gd, deterministic=True) for _ in range(2)]
    return c, ref, _check_grads(c, ref, atomic, dets, name)


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E", "F", "G", "H", "P"])
def test_base_scene_case(name):
    _single_view(name)


@pytest.mark.parametrize("name", ["L7", "L32"])
def test_long_replay_case(name):
    _single_view(name)


def test_c32_presplit_operands_case_f():
    """Case F on the path bench.py measures: the batched preprocess makes the language rows' bf16
    hi / lo operands once (split_language), and the views backward composites from them
    (k_render_bwd_wave<C32, PRE>)."""
    c, ref = bwd_cases.case("F"), bwd_cases.reference("F")
    dev = c.scene.to("cuda")
    rs = raster_settings(c.cams[0], bg=bwd_cases.BG, sh_degree=c.sh_degree, scale_modifier=c.scale_modifier)
    pfs = dgr.preprocess_views_native([rs], dev.means3D, dev.opacities, shs=dev.shs, language_feature=dev.lang,
                                      scales=dev.scales, rotations=dev.rotations, split_language=True)
    assert pfs[0].inputs.get("language_feature_split") is not None and pfs[0].fin.language_feature_split
    dgr.binning_views_native(pfs)
    nat = dgr.render_native(pfs[0])
    _check_forward(c, nat, ref.views[0])
    g = dgr.backward_views_native([nat[4]], [_dev(c.gcol[0])], [_dev(c.glang[0])], [_dev(c.gdep[0])])
    ga = oracle_keyed(g)
    assert set(ga) == _expected_fields(c)
    bad, stats = grad_check(ga, ref.grads, ref.abs)
    print("F C32+PRE", {k: {n: float(f"{x:.2e}") for n, x in s.items()} for k, s in stats.items()})
    assert not bad, (bad, stats)


@pytest.mark.parametrize("name", ["V16", "V64"])
def test_two_views_case(name):
    """backward_views_native over 2 cameras against the oracle's per-view sum, A summed over the
    views (C = 64: the per-view per-tile launches of lsr_backward_composite_views).  The views
    entry point has no deterministic mode: the deterministic gradients are the per-view
    backward_native ones accumulated into one set of buffers."""
    c, ref = bwd_cases.case(name), bwd_cases.reference(name)
    bwd_cases.check_preconditions(name, ref)
    gcs, gls, gds = ([_dev(x) for x in xs] for xs in (c.gcol, c.glang, c.gdep))
    dev = c.scene.to("cuda")     # the views entry point wants one set of Gaussian tensors
    nats = [dgr.forward_native(raster_settings(cam, bg=bwd_cases.BG, sh_degree=c.sh_degree,
                                               scale_modifier=c.scale_modifier),
                               dev.means3D, dev.opacities, shs=dev.shs, language_feature=dev.lang,
                               scales=dev.scales, rotations=dev.rotations) for cam in c.cams]
    for v, (nat, rv) in enumerate(zip(nats, ref.views)):
        _check_forward(c, nat, rv, v)
    dets = []
    for _ in range(2):
        out = None
        for nat, gc, gl, gd in zip(nats, gcs, gls, gds):
            out = dgr.backward_native(nat[4], gc, gl, gd, out=out, accumulate=True, deterministic=True)
        dets.append(out)
    atomic = dgr.backward_views_native([nat[4] for nat in nats], gcs, gls, gds)
    _check_grads(c, ref, atomic, dets, name)
