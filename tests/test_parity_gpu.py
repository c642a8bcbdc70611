"""Parity of the HIP rasterizer (through the C ABI, liblsr.so) with the CPU oracle.

Forward contract (north star): RGB within 1e-4, language features within 1e-3 of the reference.
Against the oracle the preprocess and the contributor decisions are bit-exact (same IEEE
operation order, reproducible exp), so radii and final_T are compared exactly (the preprocess's
per-Gaussian records themselves: tests/test_preprocess_fwd_branches_gpu.py).  The native
binning drops instances that cannot contribute to their tile; the tile lists are checked to be
ordered subsequences of upstream's with every dropped entry provably inactive, and every pixel's
last contributor is the same Gaussian (check_binning_against_upstream).  Channel sums differ only
by FMA rounding.  Gradients are compared relative to the
largest magnitude of each tensor (float atomics + a different summation order), 1e-4.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # CPU container: the driver only runs these on the MI355X box
    pytest.skip("needs a GPU", allow_module_level=True)

import diff_gaussian_rasterization as dgr  # noqa: E402
import oracle  # noqa: E402
import synthetic  # noqa: E402
from helpers import axis_camera, small_case  # noqa: E402
from lsr_testutil import (check_binning_against_upstream, decode_img, decode_point_list,  # noqa: E402
                          decode_point_words, grad_err, raster_settings, run_native, run_oracle)

RGB_TOL, LANG_TOL = 1e-4, 1e-3
GRAD_TOL = 1e-4


def _assert_forward(nat, ref, C, exact_state=True):
    color, lang, radii, depth, st = nat
    np.testing.assert_array_equal(radii.cpu().numpy(), ref.radii)
    assert st.num_rendered <= ref.num_rendered
    rs = ref.state()
    if exact_state:
        H, W = color.shape[1], color.shape[2]
        check_binning_against_upstream(st, rs, W, H)
    assert np.abs(color.cpu().numpy() - ref.color).max() <= RGB_TOL
    if C > 0:
        assert np.abs(lang.cpu().numpy() - ref.lang).max() <= LANG_TOL
    assert np.abs(depth.cpu().numpy() - ref.depth).max() <= 1e-4 * max(1.0, np.abs(ref.depth).max())


@pytest.mark.parametrize("C", [0, 3, 6, 16, 32, 64])
def test_forward_matches_oracle(C):
    sc, cam = small_case(P=3000, W=128, H=96, C=C, seed=C)
    nat = run_native(sc, cam)
    ref = run_oracle(sc, cam)
    _assert_forward(nat, ref, C)


@pytest.mark.parametrize("far", [False, True])
def test_depth_sort_plans(far):
    """The depth sort's pass plan, made on the device from the kept keys' range (sort.hip): depths
    2-10 span under 2^26 key units above the minimum's 256-aligned base (low 8 bits, then two 9-bit
    passes); every 7th Gaussian moved 60x further along its ray (depths up to ~600, a ratio above
    256) takes the four 8-bit passes.  Both give upstream's per-tile order
    (check_binning_against_upstream) and the oracle's images."""
    sc, cam = small_case(P=3000, W=128, H=96, C=3, seed=21)
    if far:
        sc.means3D[::7] *= 60.0   # origin camera: same projection, 60x the depth
    nat = run_native(sc, cam)
    ref = run_oracle(sc, cam)
    z = sc.means3D[:, 2].cpu().numpy()
    vis = ref.radii > 0
    assert (z[vis].max() / z[vis].min() > 256) == far
    _assert_forward(nat, ref, 3)


def test_forward_odd_size_and_big_splats():
    # ragged tiles (W, H not multiples of 16), 10 % large Gaussians, some behind the near plane
    sc, cam = small_case(P=2500, W=131, H=77, C=8, seed=5, big_frac=0.1)
    sc.means3D[:50, 2] = torch.linspace(-1.0, 0.19, 50)
    nat = run_native(sc, cam)
    ref = run_oracle(sc, cam)
    assert (ref.radii[:50] == 0).all()
    _assert_forward(nat, ref, 8)


def test_long_tile_lists():
    """Dense tiles: 12000 wide Gaussians over a 48x32 image (6 tiles), lists of > 4096 entries
    (many FIFO refills per quadrant wave, long back-to-front replays)."""
    sc, cam = small_case(P=12000, W=48, H=32, C=3, seed=12, logscale_mean=-1.5, big_frac=0.0)
    nat = run_native(sc, cam)
    ref = run_oracle(sc, cam)
    ranges, *_ = decode_img(nat[4])
    assert int((ranges[:, 1] - ranges[:, 0]).max()) > 4096
    _assert_forward(nat, ref, 3)


def test_precomputed_paths():
    sc, cam = small_case(P=1500, W=96, H=64, C=4, seed=2)
    ref = run_oracle(sc, cam, use_precomp_cov=True)
    _assert_forward(run_native(sc, cam, use_precomp_cov=True), ref, 4)
    cols = np.random.default_rng(0).uniform(0, 1, (sc.P, 3)).astype(np.float32)
    ref = run_oracle(sc, cam, colors_precomp=cols)
    _assert_forward(run_native(sc, cam, colors_precomp=cols), ref, 4)


def test_include_feature_false_writes_zero_language():
    sc, cam = small_case(P=1000, W=64, H=64, C=6, seed=3)
    color, lang, radii, depth, st = run_native(sc, cam, include_feature=False)
    ref = run_oracle(sc, cam, include_feature=False)
    assert lang.shape == (6, 64, 64) and float(lang.abs().max()) == 0.0
    assert np.abs(color.cpu().numpy() - ref.color).max() <= RGB_TOL
    # backward: language channels off -> exactly zero language gradient (buffer pre-filled), both modes
    rng = np.random.default_rng(4)
    gc = rng.normal(size=(3, 64, 64)).astype(np.float32)
    gl = rng.normal(size=(6, 64, 64)).astype(np.float32)
    rg = ref.backward(gc, gl, None)
    for det in (False, True):
        out = dict(language_feature=torch.full((1000, 6), 7.0, device="cuda"))
        g = dgr.backward_native(st, torch.tensor(gc, device="cuda"), torch.tensor(gl, device="cuda"), None, out=out,
                                deterministic=det)
        assert float(g["language_feature"].abs().max()) == 0.0, det
        assert grad_err(g["means3D"].cpu().numpy(), rg["means3D"]) < GRAD_TOL, det
        assert grad_err(g["opacities"].cpu().numpy(), rg["opacity"]) < GRAD_TOL, det


def test_empty_and_all_culled():
    cam = axis_camera()
    for P in (0, 5):
        sc = synthetic.make_scene(max(P, 1), C=3)
        if P == 0:
            sc = synthetic.Scene(*(t[:0] for t in (sc.means3D, sc.scales, sc.rotations, sc.opacities, sc.shs, sc.lang)))
        else:
            sc.means3D[:, 2] = -1.0
        color, lang, radii, depth, st = run_native(sc, cam)
        assert st.num_rendered == 0
        bg = torch.ones(3, 1, 1, device="cuda")
        assert torch.equal(color, bg.expand_as(color))
        assert float(depth.abs().max()) == 0.0


@pytest.mark.parametrize("P,culled", [(0, False), (5, True), (2048, False), (2049, False)])
def test_deferred_count_equals_forward(P, culled):
    """The single view's deferred instance count (lsr_forward_preprocess_async, read from pinned
    memory by render_native) at the sizes where its delivery changes shape: no Gaussians, none
    visible, and one scan tile (2048) against the two-tile scan (2049).  Same images, radii and
    num_rendered as the synchronous forward, bit for bit."""
    sc, cam = small_case(P=max(P, 1), W=96, H=64, C=3, seed=40 + P % 7)
    if P == 0:
        sc = synthetic.Scene(*(t[:0] for t in (sc.means3D, sc.scales, sc.rotations, sc.opacities, sc.shs, sc.lang)))
    if culled:
        sc.means3D[:, 2] = -1.0
    dev = sc.to("cuda")
    rs = raster_settings(cam)
    kw = dict(shs=dev.shs, language_feature=dev.lang, scales=dev.scales, rotations=dev.rotations)
    ref = dgr.forward_native(rs, dev.means3D, dev.opacities, **kw)
    pf = dgr.preprocess_native(rs, dev.means3D, dev.opacities, defer_count=True, **kw)
    assert pf.num_rendered is None and pf.counted is not None
    got = dgr.render_native(pf)
    assert got[4].num_rendered == ref[4].num_rendered
    assert (ref[4].num_rendered == 0) == (P == 0 or culled)
    for name, x, y in zip(("color", "language", "radii", "depth"), ref[:4], got[:4]):
        assert x.shape == y.shape and torch.equal(x, y), name


@pytest.mark.parametrize("n", [1, 8, 9])
def test_phase_launch_counts(n):
    """One set of launches per 8 views in every phase of the batched path (lsr.h), counted by the
    library's phase timers; a single view's forward_native + backward_native runs each phase once
    and the fused preprocess backward instead of the views one."""
    from diff_gaussian_rasterization import _lib
    C = 6
    sc, _ = small_case(P=3000, W=96, H=64, C=C, seed=12, big_frac=0.05)
    dev = sc.to("cuda")
    rss = [raster_settings(c, bg=(0.3, 0.6, 0.9)) for c in synthetic.camera_batch(9, 96, 64, seed=12)[:n]]
    kw = dict(scales=dev.scales, rotations=dev.rotations, shs=dev.shs, language_feature=dev.lang)
    g = torch.Generator(device="cpu").manual_seed(4)
    gcs = [torch.randn(3, 64, 96, generator=g).cuda() for _ in rss]
    gls = [torch.randn(C, 64, 96, generator=g).cuda() for _ in rss]
    forward = ("preprocess", "depth_sort", "instance_scan", "emit", "tile_sort", "render_fwd")
    try:
        _lib.profile_enable(True)
        pfs = dgr.preprocess_views_native(rss, dev.means3D, dev.opacities, **kw)
        dgr.binning_views_native(pfs)
        res = dgr.render_views_native(pfs)
        assert all(r[4].num_rendered > 0 for r in res)   # no empty view: every phase has work
        dgr.backward_views_native([r[4] for r in res], gcs, gls)
        torch.cuda.synchronize()
        batch = {k: v[1] for k, v in _lib.profile_read().items()}
        single = None
        if n == 1:
            _lib.profile_enable(True)
            *_, st = dgr.forward_native(rss[0], dev.means3D, dev.opacities, **kw)
            assert st.num_rendered > 0
            dgr.backward_native(st, gcs[0], gls[0])
            torch.cuda.synchronize()
            single = {k: v[1] for k, v in _lib.profile_read().items()}
    finally:
        _lib.profile_enable(False)
    sets = (n + 7) // 8
    for k in forward + ("render_bwd", "preprocess_bwd_views"):
        assert batch[k] == sets, (k, batch)
    assert batch["preprocess_bwd"] == 0, batch
    if single is not None:
        for k in forward + ("render_bwd", "preprocess_bwd"):
            assert single[k] == 1, (k, single)
        assert single["preprocess_bwd_views"] == 0, single


def test_sh_degrees():
    for deg in range(4):
        sc, cam = small_case(P=800, W=64, H=48, C=0, seed=10 + deg)
        _assert_forward(run_native(sc, cam, sh_degree=deg), run_oracle(sc, cam, sh_degree=deg), 0)


def test_mark_visible():
    cam = axis_camera()
    pts = torch.tensor([[0, 0, 0.19], [0, 0, 0.21], [1, 1, 5.0], [0, 0, -3.0]], device="cuda")
    r = dgr.GaussianRasterizer(raster_settings(cam))
    assert r.markVisible(pts).cpu().tolist() == [False, True, True, False]


def _grads_vs_oracle(sc, cam, C, seed=0, with_depth=True, bg=(0.3, 0.6, 0.9)):
    rng = np.random.default_rng(seed)
    H, W = cam.image_height, cam.image_width
    gcol = rng.normal(size=(3, H, W)).astype(np.float32)
    glang = rng.normal(size=(C, H, W)).astype(np.float32) if C > 0 else None
    gdep = rng.normal(size=(1, H, W)).astype(np.float32) if with_depth else None
    nat = run_native(sc, cam, bg=bg)
    ref = run_oracle(sc, cam, bg=bg)
    st = nat[4]
    g = dgr.backward_native(st, torch.tensor(gcol, device="cuda"),
                            torch.tensor(glang, device="cuda") if glang is not None else None,
                            torch.tensor(gdep, device="cuda") if gdep is not None else None)
    rg = ref.backward(gcol, glang, gdep[0] if gdep is not None else None)
    pairs = [("means3D", "means3D"), ("means2D", "means2D"), ("colors", "colors"), ("opacities", "opacity"),
             ("scales", "scales"), ("rotations", "rotations"), ("sh", "sh")]
    if C > 0:
        pairs.append(("language_feature", "lang"))
    errs = {}
    for n, o in pairs:
        errs[n] = grad_err(g[n].cpu().numpy().reshape(rg[o].shape), rg[o])
    return errs


@pytest.mark.parametrize("C", [0, 3, 32])
def test_backward_matches_oracle(C):
    sc, cam = small_case(P=2000, W=96, H=80, C=C, seed=20 + C)
    errs = _grads_vs_oracle(sc, cam, C)
    bad = {k: v for k, v in errs.items() if not v <= GRAD_TOL}
    assert not bad, errs


def test_autograd_surface_matches_backward_native():
    sc, cam = small_case(P=1200, W=64, H=64, C=6, seed=9)
    dev = "cuda"
    rs = raster_settings(cam)
    means3D = sc.means3D.to(dev).requires_grad_(True)
    means2D = torch.zeros_like(means3D, requires_grad=True)
    shs = sc.shs.to(dev).requires_grad_(True)
    opac = sc.opacities.to(dev).requires_grad_(True)
    scales = sc.scales.to(dev).requires_grad_(True)
    rots = sc.rotations.to(dev).requires_grad_(True)
    lang = sc.lang.to(dev).requires_grad_(True)
    rast = dgr.GaussianRasterizer(raster_settings=rs)
    color, lang_img, radii, depth = rast(means3D=means3D, means2D=means2D, shs=shs, colors_precomp=None,
                                         language_feature_precomp=lang, opacities=opac, scales=scales,
                                         rotations=rots, cov3D_precomp=None)
    loss = color.square().sum() + 0.5 * lang_img.square().sum()
    loss.backward()
    for t in (means3D, means2D, shs, opac, scales, rots, lang):
        assert t.grad is not None and torch.isfinite(t.grad).all()
    assert opac.grad.shape == opac.shape and shs.grad.shape == shs.shape
    # same gradients as the direct call with dL/dcolor = 2 color, dL/dlang = lang_img
    _, _, _, _, st = run_native(sc, cam)
    g = dgr.backward_native(st, 2 * color.detach(), lang_img.detach())
    assert grad_err(means3D.grad.cpu().numpy(), g["means3D"].cpu().numpy()) < 1e-5
    assert grad_err(lang.grad.cpu().numpy(), g["language_feature"].cpu().numpy()) < 1e-5


def test_accumulate_mode_sums_views():
    sc, _ = small_case(P=1000, W=64, H=48, C=4, seed=4)
    cams = synthetic.camera_batch(3, 64, 48, seed=4)
    out, total = None, None
    for c in cams:
        *_, st = run_native(sc, c)
        gc = torch.ones(3, 48, 64, device="cuda")
        gl = torch.ones(4, 48, 64, device="cuda")
        single = dgr.backward_native(st, gc, gl)
        out = dgr.backward_native(st, gc, gl, out=out, accumulate=True)
        if total is None:
            total = {k: v.clone() for k, v in single.items() if v is not None}
        else:
            for k in total:
                total[k] += single[k]
    for k in total:
        assert grad_err(out[k].cpu().numpy(), total[k].cpu().numpy()) < 1e-5, k


def _views_forward(sc_dev, cams, include_feature=True, precomp=False):
    states = []
    for c in cams:
        rs = raster_settings(c, bg=(0.3, 0.6, 0.9), include_feature=include_feature)
        kw = dict(cov3D_precomp=sc_dev.cov3D) if precomp else dict(scales=sc_dev.scales, rotations=sc_dev.rotations)
        if precomp:
            kw["colors_precomp"] = sc_dev.colors
        else:
            kw["shs"] = sc_dev.shs
        *_, st = dgr.forward_native(rs, sc_dev.means3D, sc_dev.opacities, language_feature=sc_dev.lang, **kw)
        states.append(st)
    return states


def test_backward_views_matches_oracle_sum():
    """lsr_backward_views over 3 views == the sum of the oracle's per-view backward."""
    C = 8
    sc, _ = small_case(P=1500, W=80, H=64, C=C, seed=31)
    cams = synthetic.camera_batch(3, 80, 64, seed=31)
    states = _views_forward(sc.to("cuda"), cams)
    rng = np.random.default_rng(3)
    gcs = [rng.normal(size=(3, 64, 80)).astype(np.float32) for _ in cams]
    gls = [rng.normal(size=(C, 64, 80)).astype(np.float32) for _ in cams]
    g = dgr.backward_views_native(states, [torch.tensor(x, device="cuda") for x in gcs],
                                  [torch.tensor(x, device="cuda") for x in gls])
    total = None
    for c, gc, gl in zip(cams, gcs, gls):
        rg = run_oracle(sc, c, bg=(0.3, 0.6, 0.9)).backward(gc, gl, None)
        total = {k: v.astype(np.float64) for k, v in rg.items()} if total is None else \
            {k: total[k] + rg[k] for k in total}
    pairs = [("means3D", "means3D"), ("means2D", "means2D"), ("colors", "colors"), ("opacities", "opacity"),
             ("scales", "scales"), ("rotations", "rotations"), ("sh", "sh"), ("language_feature", "lang")]
    errs = {n: grad_err(g[n].cpu().numpy().reshape(total[o].shape), total[o]) for n, o in pairs}
    assert all(e <= GRAD_TOL for e in errs.values()), errs


@pytest.mark.parametrize("precomp", [False, True])
def test_backward_views_equals_per_view_sum(precomp):
    """10 views (two launches of the 8-view kernel), accumulating onto existing buffers: equal to
    the per-view lsr_backward sum.  precomp: colors_precomp + cov3D_precomp (no SH rows)."""
    C = 4
    sc, _ = small_case(P=1200, W=64, H=48, C=C, seed=8)
    dev = sc.to("cuda")
    if precomp:
        dev.cov3D = torch.tensor(oracle.cov3d(sc.scales.numpy(), sc.rotations.numpy())).cuda()
        dev.colors = torch.rand(sc.means3D.shape[0], 3, generator=torch.Generator().manual_seed(1)).cuda()
    cams = synthetic.camera_batch(10, 64, 48, seed=8)
    states = _views_forward(dev, cams, precomp=precomp)
    g = torch.Generator(device="cpu").manual_seed(2)
    gcs = [torch.randn(3, 48, 64, generator=g).cuda() for _ in cams]
    gls = [torch.randn(C, 48, 64, generator=g).cuda() for _ in cams]
    base = None
    ref = None
    for st, gc, gl in zip(states, gcs, gls):
        one = dgr.backward_native(st, gc, gl)
        if base is None:
            base = {k: torch.randn_like(v) for k, v in one.items() if v is not None}
            ref = {k: v.clone() for k, v in base.items()}
        for k in ref:
            ref[k] += one[k]
    out = {k: v.clone() for k, v in base.items()}
    got = dgr.backward_views_native(states, gcs, gls, out=out, accumulate=True)
    for k in ref:
        assert got[k] is out[k]
        assert grad_err(got[k].cpu().numpy(), ref[k].cpu().numpy()) <= 1e-5, k
    with pytest.raises(RuntimeError, match="deterministic"):
        import ctypes
        from diff_gaussian_rasterization import _lib
        L = _lib.load()
        gi = _lib.BwdIn()
        gi.dL_dout_color, gi.deterministic = gcs[0].data_ptr(), 1
        st = states[0]
        SP, BP = ctypes.POINTER(_lib.Settings), ctypes.POINTER(_lib.BwdIn)
        vp = ctypes.c_void_p * 1
        gout = _lib.BwdOut()
        _lib.check(L.lsr_backward_views(1, (SP * 1)(ctypes.pointer(st.settings.c)), ctypes.byref(st.fin),
                                        (BP * 1)(ctypes.pointer(gi)), ctypes.byref(gout), vp(st.geom.data_ptr()),
                                        vp(st.binning.data_ptr()), vp(st.img.data_ptr()),
                                        (ctypes.c_int64 * 1)(st.num_rendered), 0, None), "lsr_backward_views")



@pytest.mark.parametrize("precomp", [False, True])
def test_batched_forward_equals_per_view(precomp):
    """lsr_forward_preprocess_views_async + lsr_forward_binning_views over 10 views (an 8-view and a
    2-view launch set; one camera sees nothing): every output, the point lists, the tile ranges and
    final T / n_contrib equal the per-view forward bit for bit, and the batched backward matches."""
    C = 6
    sc, _ = small_case(P=2000, W=96, H=64, C=C, seed=12, big_frac=0.05)
    dev = sc.to("cuda")
    if precomp:
        dev.cov3D = torch.tensor(oracle.cov3d(sc.scales.numpy(), sc.rotations.numpy())).cuda()
        dev.colors = torch.rand(sc.means3D.shape[0], 3, generator=torch.Generator().manual_seed(1)).cuda()
    cams = synthetic.camera_batch(10, 96, 64, seed=12)
    rss = [raster_settings(c, bg=(0.3, 0.6, 0.9)) for c in cams]
    away = cams[3].world_view_transform.clone()
    away[3, 2] -= 1000.0                   # view 3: every Gaussian behind the near plane, K = 0
    rss[3] = rss[3]._replace(viewmatrix=away.to("cuda"))
    kw = dict(cov3D_precomp=dev.cov3D, colors_precomp=dev.colors) if precomp else dict(
        scales=dev.scales, rotations=dev.rotations, shs=dev.shs)
    ref = [dgr.forward_native(rs, dev.means3D, dev.opacities, language_feature=dev.lang, **kw) for rs in rss]
    pfs = dgr.preprocess_views_native(rss, dev.means3D, dev.opacities, language_feature=dev.lang, **kw)
    dgr.binning_views_native(pfs)
    got = [dgr.render_native(pf) for pf in pfs]
    assert ref[3][4].num_rendered == 0 and got[3][4].num_rendered == 0
    for v, (a, b) in enumerate(zip(ref, got)):
        assert a[4].num_rendered == b[4].num_rendered, v
        for x, y in zip(a[:4], b[:4]):
            assert torch.equal(x, y), v
        if a[4].num_rendered:   # the listed entries (the unlisted are dropped by the tile sort)
            n = int(decode_img(a[4])[0][:, 1].max())
            assert np.array_equal(decode_point_list(a[4])[:n], decode_point_list(b[4])[:n]), v
        for x, y in zip(decode_img(a[4]), decode_img(b[4])):
            assert np.array_equal(x, y), v
    g = torch.Generator(device="cpu").manual_seed(4)
    gcs = [torch.randn(3, 64, 96, generator=g).cuda() for _ in cams]
    gls = [torch.randn(C, 64, 96, generator=g).cuda() for _ in cams]
    ga = dgr.backward_views_native([r[4] for r in ref], gcs, gls)
    gb = dgr.backward_views_native([r[4] for r in got], gcs, gls)
    for k in ga:
        if ga[k] is not None:
            assert grad_err(gb[k].cpu().numpy(), ga[k].cpu().numpy()) <= 1e-5, k

def test_full_size_forward_matches_oracle():
    """Headline size (1352 x 1014, C = 32) at 400k Gaussians: exact lists, bit-exact T."""
    sc = synthetic.make_scene(400_000, C=32)
    cam = synthetic.origin_camera()
    nat = run_native(sc, cam)
    ref = run_oracle(sc, cam, nthreads=16)
    _assert_forward(nat, ref, 32)


def test_config1_rgb_only_forward_and_backward():
    """BASELINE.json configs[0] at full size: 50k Gaussians, one 400 x 400 camera (tanfov 0.6 / 0.6),
    3 channels with include_feature=False and a zeros language tensor (gaussian_renderer/__init__.py:
    96-99).  Exact lists and radii, RGB within 1e-4, language output and gradient exactly zero, every
    other gradient within 1e-4 of the oracle."""
    W = H = 400
    sc = synthetic.make_scene(50_000, C=3, tanfovx=0.6, tanfovy=0.6, seed=0)
    sc.lang = torch.zeros_like(sc.lang)
    cam = synthetic.origin_camera(W, H, tanfovx=0.6, tanfovy=0.6)
    nat = run_native(sc, cam, include_feature=False)
    ref = run_oracle(sc, cam, include_feature=False, nthreads=16)
    _assert_forward(nat, ref, 0)
    assert float(nat[1].abs().max()) == 0.0
    rng = np.random.default_rng(7)
    gc = rng.normal(size=(3, H, W)).astype(np.float32)
    g = dgr.backward_native(nat[4], torch.tensor(gc, device="cuda"), None, None)
    rg = ref.backward(gc, None, None, nthreads=16)
    for n, o in (("means3D", "means3D"), ("means2D", "means2D"), ("opacities", "opacity"), ("scales", "scales"),
                 ("rotations", "rotations"), ("sh", "sh")):
        assert grad_err(g[n].cpu().numpy().reshape(rg[o].shape), rg[o]) <= GRAD_TOL, n
    assert float(g["language_feature"].abs().max()) == 0.0


def test_config2_render_forward():
    """BASELINE.json configs[1] stand-in (the pretrained americano scene is unavailable
    offline): 300k Gaussians, 960 x 540, RGB + 3 language channels with include_feature=True,
    forward only as render.py runs it.  Exact lists and radii; RGB 1e-4, language 1e-3."""
    W, H = 960, 540
    sc = synthetic.make_scene(300_000, C=3, tanfovx=0.6, tanfovy=0.6 * H / W, seed=2)
    cam = synthetic.origin_camera(W, H)
    with torch.no_grad():
        nat = run_native(sc, cam)
    ref = run_oracle(sc, cam, nthreads=16)
    _assert_forward(nat, ref, 3)


def test_headline_properties_2m():
    """2M Gaussians: size-independent invariants (sorted per-tile lists, counts, saturation)."""
    sc = synthetic.make_scene(2_000_000, C=32)
    cam = synthetic.origin_camera()
    color, lang, radii, depth, st = run_native(sc, cam)
    ranges, tmax, fT, nc = decode_img(st)
    pl = decode_point_list(st).astype(np.int64)
    vis = radii.cpu().numpy() > 0
    assert 1_500_000 < vis.sum() < 1_950_000
    K = st.num_rendered
    assert 4_000_000 < K < 12_000_000        # after dropping instances that cannot contribute
    # ranges tile the list in order; the instances reaching no quadrant of their tile are dropped
    nz = ranges[:, 1] > ranges[:, 0]
    listed = int(ranges[nz, 1].sum() - ranges[nz, 0].sum())
    assert 0.5 * K < listed <= K and int(ranges[nz, 1].max()) == listed
    # inside each tile: strictly increasing (depth, id)
    depthv = sc.means3D[:, 2].numpy()  # origin camera: view z == world z
    for t in np.random.default_rng(0).choice(np.nonzero(nz)[0], 64, replace=False):
        ids = pl[ranges[t, 0]:ranges[t, 1]]
        d = depthv[ids]
        assert (np.diff(d) >= 0).all()
        ties = np.diff(d) == 0
        assert (np.diff(ids)[ties] > 0).all()
    assert (fT >= 0).all() and (fT <= 1).all()
    assert (nc <= (ranges[:, 1] - ranges[:, 0]).max()).all()
    assert torch.isfinite(color).all() and torch.isfinite(lang).all()


def test_deterministic_backward_is_bitwise_reproducible():
    sc, cam = small_case(P=3000, W=128, H=96, C=32, seed=31)
    rng = np.random.default_rng(1)
    gc = torch.tensor(rng.normal(size=(3, 96, 128)).astype(np.float32), device="cuda")
    gl = torch.tensor(rng.normal(size=(32, 96, 128)).astype(np.float32), device="cuda")
    *_, st = run_native(sc, cam)
    g1 = dgr.backward_native(st, gc, gl, deterministic=True)
    g2 = dgr.backward_native(st, gc, gl, deterministic=True)
    ga = dgr.backward_native(st, gc, gl, deterministic=False)
    for k, v in g1.items():
        if v is None:
            continue
        assert torch.equal(v, g2[k]), k
        # the default path sums over pixels on matrix cores (bf16 x3 products, ~1e-5 relative);
        # both modes are held to the oracle at 1e-4 below and in test_backward_matches_oracle
        assert grad_err(ga[k].cpu().numpy(), v.cpu().numpy()) < 5e-5, k
    # and the deterministic gradients match the oracle like the default ones
    ref = run_oracle(sc, cam)
    rg = ref.backward(gc.cpu().numpy(), gl.cpu().numpy(), None)
    for n, o in (("means3D", "means3D"), ("language_feature", "lang"), ("opacities", "opacity"), ("sh", "sh")):
        assert grad_err(g1[n].cpu().numpy().reshape(rg[o].shape), rg[o]) <= GRAD_TOL, n


def test_split_backward_runs_once_per_forward():
    """lsr_backward_composite adds into the forward's accumulator rows: a second run on the same
    forward would double them, so the wrapper refuses it."""
    C = 8
    sc, cam = small_case(P=1500, W=96, H=64, C=C, seed=3)
    dev = "cuda"
    rs = raster_settings(cam)
    color, lang, radii, depth, st = dgr.forward_native(rs, sc.means3D.to(dev), sc.opacities.to(dev),
                                                       shs=sc.shs.to(dev), language_feature=sc.lang.to(dev),
                                                       scales=sc.scales.to(dev), rotations=sc.rotations.to(dev))
    assert torch.isfinite(color).all()
    dl = torch.zeros(sc.means3D.shape[0], C, device=dev)
    dgr.backward_composite_native(st, torch.ones_like(color), torch.ones_like(lang), dL_dlanguage=dl)
    with pytest.raises(RuntimeError, match="already ran"):
        dgr.backward_composite_native(st, torch.ones_like(color), torch.ones_like(lang), dL_dlanguage=dl)


@pytest.mark.parametrize("seed,big", [(21, 0.0), (22, 0.2)])
def test_quadrant_bits_are_conservative(seed, big):
    """Every quadrant bit the binning clears (k_emit, emit_quad_mask) belongs to a quadrant where
    the splat's alpha stays below 1/255 at every pixel (float64 evaluation of the oracle's
    screen-space splat), so the compositors' per-quadrant scans skip nothing that blends."""
    W, H = 203, 141
    sc, cam = small_case(P=4000, W=W, H=H, C=3, seed=seed, big_frac=big)
    nat = run_native(sc, cam)
    ref = run_oracle(sc, cam).state()
    st = nat[4]
    ranges, *_ = decode_img(st)
    words = decode_point_words(st).astype(np.int64)
    xy, co = ref["xy"].astype(np.float64), ref["conic_o"].astype(np.float64)
    gx = (W + 15) // 16
    checked = cleared = 0
    for t in range(len(ranges)):
        wv = words[ranges[t, 0]:ranges[t, 1]]
        if len(wv) == 0:
            continue
        gid, bits = wv & 0x0FFFFFFF, wv >> 28
        assert (bits != 0).all()            # instances reaching no quadrant are not listed
        tx, ty = t % gx, t // gx
        for q in range(4):
            x0, y0 = 16 * tx + 8 * (q & 1), 16 * ty + 8 * (q >> 1)
            if x0 >= W or y0 >= H:
                continue
            off = ((bits >> q) & 1) == 0
            checked += len(wv)
            if not off.any():
                continue
            g = gid[off]
            cleared += len(g)
            px, py = np.meshgrid(np.arange(x0, min(x0 + 8, W)), np.arange(y0, min(y0 + 8, H)))
            dx = xy[g, 0][:, None] - px.ravel()[None]
            dy = xy[g, 1][:, None] - py.ravel()[None]
            a, b, c, o = (co[g, k][:, None] for k in range(4))
            power = -0.5 * (a * dx * dx + c * dy * dy) - b * dx * dy
            alpha = np.minimum(0.99, o * np.exp(np.minimum(power, 0.0)))
            assert (alpha < (1.0 / 255.0) * (1 - 1e-6)).all(), (t, q)
    assert checked > 0 and cleared > 0.05 * checked    # the bits do prune
