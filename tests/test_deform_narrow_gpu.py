"""The deformation field at net_width 64 / output_coordinate_dim 32 on the GPU (csrc/deform_narrow.hip
through include/lsr_deform.h): against the reference module's outputs and autograd
(tests/golden/deform_narrow_{variant}.npz), the float64 oracle on shapes the fixture lacks, the ABI's
refusals, and a model directory, a training step and the plane regularisers end to end."""
import ctypes
import os

import numpy as np
import pytest
import torch

from deform_oracle import DeformConfig, DeformOracle
from deformation import HEADS, HEAD_OUT, LANG_PASS, LANG_RESIDUAL, DeformationField
from lsr_testutil import DEFORM_COEF, U24, deform_check
from test_deform_gpu import _morton
from test_deform_narrow import VARIANTS, load_variant

pytestmark = pytest.mark.gpu
KEYS = ("means3D", "scales", "rotations", "opacity", "shs")
NAMES = KEYS + ("lang",)
RES = [6, 5, 4, 7]
COMBOS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _t(a):
    return None if a is None else torch.tensor(np.asarray(a, np.float32)).cuda()


def _variant_field(name):
    cfg, dc, params, grads, d = load_variant(name)
    p = {k: torch.tensor(v).cuda() for k, v in params.items()}
    p["grid.aabb"] = torch.tensor(d["aabb"]).cuda()
    f = DeformationField(p, cfg["res"], cfg["multires"], depth=cfg["depth"], no_dx=cfg["no_dx"], no_ds=cfg["no_ds"],
                         no_dr=cfg["no_dr"], no_do=cfg["no_do"], no_dshs=cfg["no_dshs"],
                         apply_rotation=cfg["apply_rotation"], lang_mode=LANG_PASS, lang_dim=cfg["lang_dim"])
    assert (f.channels, f.width) == (32, 64)
    return f, cfg, dc, params, grads, d


# ---- the reference's fixture ---------------------------------------------------------------------
@pytest.mark.parametrize("name", VARIANTS)
def test_forward_matches_reference(name):
    """Every output against the reference module: residual outputs as offsets (what the kernels
    compute) within 1e-4 of each output's range; a head that is off returns its input bit for bit."""
    f, cfg, _, _, _, d = _variant_field(name)
    out = f.forward(*[_t(d[k]) for k in NAMES], _t(d["time"])[:, 0])
    assert out[6] is None
    for k, o in zip(NAMES, out):
        ref = d["out_" + k].astype(np.float64)
        got = o.cpu().numpy().astype(np.float64).reshape(ref.shape)
        base = d[k].astype(np.float64).reshape(ref.shape)
        if k == "lang" or np.abs(ref - base).max() == 0:       # passed through / head off: the input itself
            assert np.array_equal(got, base), k
        elif k == "rotations" and cfg["apply_rotation"]:
            assert _rel(got, ref) < 1e-4, k
        else:
            assert _rel(got - base, ref - base) < 1e-4, k


@pytest.mark.parametrize("name", VARIANTS)
def test_backward_matches_reference(name):
    """The procedure of test_variant_backward_matches_reference: against the reference-pinned oracle
    within 1e-4 once the upstream of the Gaussians with a ReLU input within 1e-4 of zero is zeroed
    (fewer than half), against the reference's autograd on the full upstream within 5e-2 of each
    tensor's range (kink flips), the gradient keys are the fixture's, and a second backward without
    zero_grad doubles every parameter gradient (accumulation)."""
    f, cfg, dc, params, ref_grads, d = _variant_field(name)

    def run(ups, twice=False):
        f.zero_grad()
        for _ in range(2 if twice else 1):
            got = f.backward(_t(d["means3D"]), _t(d["time"])[:, 0], *[_t(ups[k]) for k in KEYS],
                             rotations=_t(d["rotations"]), lang=_t(d["lang"]), d_lang=_t(ups["lang"]))
        torch.cuda.synchronize()
        return [g.cpu().numpy() for g in got], {k: v.cpu().numpy() for k, v in f.grads.items()}

    o = DeformOracle(params, d["aabb"], cfg=dc)
    f64 = lambda k: d[k].astype(np.float64)   # noqa: E731
    o.forward(*[f64(k) for k in NAMES], f64("time"))
    amb = np.zeros(d["means3D"].shape[0], bool)
    for v in o.preactivations():
        amb |= (np.abs(v) < 1e-4).any(axis=1)
    assert amb.mean() < 0.5
    ups = {k: d["up_" + k].copy() for k in NAMES}
    for v in ups.values():
        v[amb] = 0.0
    g_in, g_p = o.backward(*[ups[k].astype(np.float64) for k in KEYS], up_lang=ups["lang"].astype(np.float64))
    got, grads = run(ups)
    for k, g in zip(NAMES, got):
        assert _rel(g.reshape(g_in[k].shape), g_in[k]) < 1e-4, k
    assert set(grads) == set(g_p)
    for k, v in g_p.items():
        assert _rel(grads[k].reshape(v.shape), v) < 1e-4, k
    _, twice = run(ups, twice=True)
    for k, v in g_p.items():
        assert _rel(twice[k].reshape(v.shape) / 2.0, v) < 1e-4, k
        assert _rel(twice[k], 2.0 * grads[k]) < 1e-5, k          # atomics: the order differs run to run
    # every Gaussian: the reference's own gradients, up to the kink flips
    got, grads = run({k: d["up_" + k] for k in NAMES})
    assert set(grads) == set(ref_grads)
    for k, g in zip(NAMES, got):
        assert _rel(g.reshape(d["grad_" + k].shape), d["grad_" + k]) < 5e-2, k
    for k, v in ref_grads.items():
        assert _rel(grads[k].reshape(v.shape), v) < 5e-2, k


def test_apply_gives_the_gradients_of_backward():
    f, cfg, _, _, _, d = _variant_field("full")
    xs = [_t(d[k]).requires_grad_(True) for k in NAMES]
    time = _t(d["time"])[:, 0]
    outs = f.apply(*xs, time)
    ref = f.forward(*[x.detach() for x in xs], time)
    for a, b in zip(outs[:5], ref[:5]):
        assert torch.equal(a.detach(), b)
    f.zero_grad()
    sum((o * _t(d["up_" + k]).reshape(o.shape)).sum() for o, k in zip(outs[:6], NAMES)).backward()
    auto = {k: v.clone() for k, v in f.grads.items()}
    f.zero_grad()
    want = f.backward(_t(d["means3D"]), time, *[_t(d["up_" + k]) for k in KEYS], rotations=_t(d["rotations"]),
                      lang=_t(d["lang"]), d_lang=_t(d["up_lang"]))
    for x, r, k in zip(xs, want, NAMES):
        assert _rel(x.grad.cpu().numpy(), r.cpu().numpy().reshape(x.shape)) < 1e-6, k
    for k, v in f.grads.items():
        assert _rel(auto[k].cpu().numpy(), v.cpu().numpy()) < 1e-5, k   # float atomics in another order


# ---- shapes the fixture lacks, against the oracle on seeded random parameters ----------------------
def _random_case(multires, P, depth=1, heads=(True, True, True, True, True), apply_rotation=False, seed=0):
    rng = np.random.default_rng(seed)
    S = len(multires)
    params = {}
    for s, m in enumerate(multires):
        rs = [r * m for r in RES[:3]] + [RES[3]]
        for ci, (c0, c1) in enumerate(COMBOS):
            params[f"grid.grids.{s}.{ci}"] = rng.uniform(0.1, 1.5, size=(1, 32, rs[c1], rs[c0]))
    for k in range(max(depth, 1)):
        params[f"feature_out.{2 * k}.weight"] = rng.normal(scale=0.2, size=(64, 32 * S if k == 0 else 64))
        params[f"feature_out.{2 * k}.bias"] = rng.normal(scale=0.05, size=64)
    for name, n, on in zip(HEADS, HEAD_OUT, heads):
        if on:
            params[name + ".1.weight"] = rng.normal(scale=0.15, size=(64, 64))
            params[name + ".1.bias"] = rng.normal(scale=0.05, size=64)
            params[name + ".3.weight"] = rng.normal(scale=0.15, size=(n, 64))
            params[name + ".3.bias"] = rng.normal(scale=0.05, size=n)
    params = {k: np.asarray(v, np.float32).astype(np.float64) for k, v in params.items()}
    aabb = np.array([[1.5, 1.2, 3.0], [-1.4, -1.1, 0.5]], np.float32).astype(np.float64)
    lo, hi = aabb[1], aabb[0]
    ext = 0.15 * (hi - lo)                                   # some points outside the box: border clamp
    inp = dict(means3D=rng.uniform(lo - ext, hi + ext, size=(P, 3)), scales=rng.normal(-4, 0.5, size=(P, 3)),
               rotations=rng.normal(size=(P, 4)), opacity=rng.normal(size=(P, 1)),
               shs=rng.normal(scale=0.3, size=(P, 16, 3)))
    # keep the points 1e-3 cells away from every grid line, where float32 and float64 coordinates
    # could pick different cells (as test_backward_matches_oracle_at_neu3d_resolution)
    inp = {k: np.asarray(v, np.float32).astype(np.float64) for k, v in inp.items()}

    def near_a_line():
        crd = (inp["means3D"] - aabb[0]) * (2.0 / (aabb[1] - aabb[0])) - 1.0
        bad = np.zeros((P, 3), bool)
        for m in multires:
            u = (crd + 1.0) * 0.5 * (np.array(RES[:3]) * m - 1)
            bad |= np.abs(u - np.round(u)) <= 1e-3
        return bad
    for _ in range(8):
        bad = near_a_line()
        if not bad.any():
            break
        moved = inp["means3D"] + bad * 0.013 * (hi - lo) / (np.array(RES[:3]) * multires[-1])
        inp["means3D"] = np.asarray(moved, np.float32).astype(np.float64)
    assert not near_a_line().any()
    times = rng.uniform(-1.2, 1.2, size=(P, 1))
    times[::3] = 1.0                                          # exactly on the clamped border rows
    times[1::3] = -1.0
    times = np.asarray(times, np.float32).astype(np.float64)
    ups = dict(means3D=rng.normal(size=(P, 3)), scales=rng.normal(size=(P, 3)), rotations=rng.normal(size=(P, 4)),
               opacity=rng.normal(size=(P, 1)), shs=rng.normal(size=(P, 16, 3)) * 0.1)
    ups = {k: np.asarray(v, np.float32).astype(np.float64) for k, v in ups.items()}
    cfg = DeformConfig(n_scales=S, depth=depth, heads=heads, apply_rotation=apply_rotation)
    return params, aabb, inp, times, ups, cfg


def _check_against_oracle(multires, P, morton=False, **kw):
    params, aabb, inp, times, ups, cfg = _random_case(multires, P, **kw)
    if morton:
        order = _morton(inp["means3D"])
        inp = {k: v[order] for k, v in inp.items()}
        times[:] = 0.37                                       # one time, as a rendered view
    heads = cfg.heads
    p = {k: _t(v) for k, v in params.items()}
    p["grid.aabb"] = _t(aabb)
    f = DeformationField(p, RES, multires, depth=cfg.depth, no_dx=not heads[0], no_ds=not heads[1],
                         no_dr=not heads[2], no_do=not heads[3], no_dshs=not heads[4],
                         apply_rotation=cfg.apply_rotation)
    f.train_aabb = True
    o = DeformOracle(params, aabb, cfg=cfg)
    ref = o.forward(*[inp[k] for k in KEYS], None, times)
    out = f.forward(*[_t(inp[k]) for k in KEYS], None, _t(times[:, 0]))
    rng_of = lambda a: max(np.abs(a).max(), 1e-30)   # noqa: E731
    for k, g, on in zip(KEYS, out, heads):
        got = g.cpu().numpy().astype(np.float64).reshape(inp[k].shape)
        if not on:
            assert np.array_equal(got, inp[k]), k
        elif k == "rotations" and cfg.apply_rotation:
            assert np.abs(got - ref[k]).max() < 1e-4 * rng_of(ref[k]), k
        else:
            # one Gaussian has no range of its own: the offsets' scale is that of the head's outputs
            assert np.abs((got - inp[k]) - (ref[k] - inp[k])).max() < 1e-4 * rng_of(ref[k] - inp[k]), k
    amb = np.zeros(P, bool)
    for v in o.preactivations():
        amb |= (np.abs(v) < 1e-4).any(axis=1)
    assert amb.mean() < 0.5 if P >= 10 else not amb.all()      # the backward comparison below always runs
    for v in ups.values():
        v[amb] = 0.0
    g_in, g_p = o.backward(*[ups[k] for k in KEYS])
    f.zero_grad()
    got = f.backward(_t(inp["means3D"]), _t(times[:, 0]), *[_t(ups[k]) for k in KEYS], rotations=_t(inp["rotations"]))
    torch.cuda.synchronize()
    assert _rel(got[0].cpu().numpy(), g_in["means3D"]) < 1e-4
    if cfg.apply_rotation:
        assert _rel(got[2].cpu().numpy(), g_in["rotations"]) < 1e-4
    grads = {k: v.cpu().numpy() for k, v in f.grads.items()}
    assert set(grads) == set(g_p) | {"grid.aabb"}
    for k, v in g_p.items():
        assert _rel(grads[k].reshape(v.shape), v) < 1e-4, k
    # the box: n = (p - a0) s - 1, s = 2 / (a1 - a0), dL/dp = dL/dn s through the coordinates, so
    # dL/da0 = sum dL/dp (n - 1) / 2 and dL/da1 = -sum dL/dp (n + 1) / 2 (hexplane.py normalize_aabb)
    gq = g_in["means3D"] - ups["means3D"]
    n = (inp["means3D"] - aabb[0]) * (2.0 / (aabb[1] - aabb[0])) - 1.0
    want = np.stack([(0.5 * gq * (n - 1.0)).sum(0), (-0.5 * gq * (n + 1.0)).sum(0)])
    assert _rel(grads["grid.aabb"], want) < 1e-4
    # per element as well (lsr_testutil.deform_check, as tests/test_deform_branches_gpu.py): against the oracle
    # on the kernels' float32 cells, with its term scales, the same masked upstream, and its box gradient
    o32 = DeformOracle(params, aabb, cfg=cfg, coords="float32", train_aabb=True)
    r32, A_out = o32.forward(*[inp[k] for k in KEYS], None, times, abs_terms=True)
    g_in32, g_p32, A_in, A_p = o32.backward(*[ups[k] for k in KEYS], abs_terms=True)
    plain = [k for k in KEYS if not (k == "rotations" and cfg.apply_rotation)]
    nat = {k: g.cpu().numpy().astype(np.float64).reshape(inp[k].shape) for k, g in zip(KEYS, out)}
    for k in KEYS:   # a stored residual output fl(input + offset) carries that one rounding beside coef A
        A_out[k] = A_out[k] + (A_out[k] > 0) * (U24 / DEFORM_COEF) * np.abs(r32[k])
    bad, _ = deform_check({k: nat[k] - inp[k] if k in plain else nat[k] for k in KEYS},
                          {k: r32[k] - inp[k] if k in plain else r32[k] for k in KEYS}, A_out)
    assert not bad, bad
    nat_in = {"means3D": got[0].cpu().numpy()}
    if cfg.apply_rotation:
        nat_in["rotations"] = got[2].cpu().numpy()
    bad, _ = deform_check(nat_in, g_in32, A_in)
    assert not bad, bad
    assert set(grads) == set(g_p32)
    bad, _ = deform_check(grads, g_p32, A_p)
    assert not bad, bad
    assert _rel(grads["grid.aabb"], g_p32["grid.aabb"]) < 1e-4
    return f


@pytest.mark.parametrize("P", (1, 65, 300))
@pytest.mark.parametrize("multires", ([1], [1, 2, 4]), ids=("S1", "S3"))
def test_other_scale_counts_and_sizes_match_oracle(multires, P):
    """S = 1 and S = 3; one Gaussian, one past a 64-row block, a ragged tail; times exactly +-1 and
    points outside the box; forward and backward within 1e-4."""
    _check_against_oracle(multires, P, depth=1, seed=7 + P)


@pytest.mark.parametrize("depth,heads,rot", [(0, (True, False, True, False, True), True),
                                             (4, (False, True, False, True, False), False),
                                             (3, (True, True, True, True, True), True)])
def test_depths_and_head_masks_match_oracle(depth, heads, rot):
    _check_against_oracle([1, 2], 130, depth=depth, heads=heads, apply_rotation=rot, seed=11 + depth)


def test_large_morton_ordered_call_matches_oracle_and_repeats():
    """P = 20,000 along a Morton curve at one time: back-to-back atomics into the same plane cells,
    more blocks than CUs.  The forward of the same call repeated is bit-identical."""
    P = 20000
    f = _check_against_oracle([1, 2], P, morton=True, depth=0, heads=(True, True, True, False, False), seed=3)
    rng = np.random.default_rng(1)
    ins = [_t(rng.normal(size=(P,) + s)) for s in ((3,), (3,), (4,), (1,), (16, 3))]
    a = f.forward(*ins, None, 0.37)
    b = f.forward(*ins, None, 0.37)
    torch.cuda.synchronize()
    for x, y in zip(a[:5], b[:5]):
        assert torch.equal(x, y)


# ---- the ABI -------------------------------------------------------------------------------------
def test_abi_refuses_other_shapes_and_the_centres():
    from diff_gaussian_rasterization import _lib
    L = _lib.load()
    p = DeformationField.init_params(RES, [1, 2], [[1, 1, 1], [-1, -1, -1]], channels=32, width=64)
    f = DeformationField({k: v.cuda() for k, v in p.items()}, RES, [1, 2], no_do=False, no_dshs=False)
    wide_p = DeformationField.init_params(RES, [1, 2], [[1, 1, 1], [-1, -1, -1]])
    wide = DeformationField({k: v.cuda() for k, v in wide_p.items()}, RES, [1, 2], no_do=False, no_dshs=False)
    n_narrow = int(L.lsr_deform_workspace_bytes(ctypes.byref(f.net)))
    n_wide = int(L.lsr_deform_workspace_bytes(ctypes.byref(wide.net)))
    assert n_narrow > 0 and n_wide > 0 and n_narrow != n_wide
    assert int(L.lsr_deform_backward_scratch_bytes(ctypes.byref(f.net), 100)) > 0
    P = 8
    x = [torch.zeros(P, *s, device="cuda") for s in ((3,), (3,), (4,), (1,), (16, 3))]
    outs = [torch.full_like(t, 7.0) for t in x]
    tm = torch.zeros(P, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)   # noqa: E731
    for ch, w in ((16, 64), (32, 128)):
        net = f._net(LANG_PASS)
        net.channels, net.width = ch, w
        assert int(L.lsr_deform_workspace_bytes(ctypes.byref(net))) == -1
        assert int(L.lsr_deform_backward_scratch_bytes(ctypes.byref(net), P)) == -1
        rc = L.lsr_deform_forward(ctypes.byref(net), vp(f.workspace), P, *[vp(t) for t in x], vp(None), vp(tm),
                                  *[vp(t) for t in outs], vp(None), vp(None), ctypes.c_void_p(0))
        assert rc == 1                                               # LSR_EINVAL (include/lsr.h)
        assert b"32 channels" in L.lsr_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs)               # nothing ran
    # a language mode without kernels at this shape: the message names the mode and the shape
    net = f._net(LANG_RESIDUAL)
    assert int(L.lsr_deform_workspace_bytes(ctypes.byref(net))) == -1
    msg = L.lsr_last_error()
    assert b"RESIDUAL" in msg and b"32 channels / width 64" in msg
    p_lang = DeformationField.init_params(RES, [1, 2], [[1, 1, 1], [-1, -1, -1]], channels=32, width=64,
                                          lang_mode=LANG_RESIDUAL)
    with pytest.raises(ValueError, match="RESIDUAL.*32.*64"):
        DeformationField({k: v.cuda() for k, v in p_lang.items()}, RES, [1, 2], no_do=False, no_dshs=False,
                         lang_mode=LANG_RESIDUAL)
    # the centres: refused by the library and by the Python entry points
    import language_centers as lc
    lang = torch.randn(P, 3, device="cuda")
    with pytest.raises(ValueError, match="32"):
        lc.sample_centers(f, lang, k=2, samples=8)
    cen, cnt, inertia, iters = (torch.zeros(P, 2, 3, device="cuda"), torch.zeros(P, 2, dtype=torch.int32, device="cuda"),
                                torch.zeros(P, device="cuda"), torch.zeros(P, dtype=torch.int32, device="cuda"))
    rc = L.lsr_centers_from_field(ctypes.byref(f.net), vp(f.workspace), P, vp(lang), vp(None), 0, 8, 2, 10, vp(cen),
                                  vp(cnt), vp(inertia), vp(iters), vp(None), vp(None), ctypes.c_void_p(0))
    assert rc != 0 and b"32 channels" in L.lsr_last_error()


# ---- end to end ------------------------------------------------------------------------------------
W, H = 96, 72
AABB = [[7.0, 5.5, 10.5], [-7.0, -5.5, 1.5]]
LRS = {"xyz": 1.6e-4, "f_dc": 2.5e-2, "f_rest": 2.5e-2 / 20, "opacity": 0.05, "scaling": 5e-3, "rotation": 1e-3}
DNERF_HEADS = ("pos_deform", "scales_deform", "rotations_deform")


def test_model_directory_round_trip(tmp_path):
    """save_model_dir then load_model_dir of a scene with a dnerf-shaped field (the hidden parameters
    come from deformation_config.json, which records the field's own net_width and
    output_coordinate_dim): the loaded field's forward is the original's bit for bit, and both render
    the same fine-base image."""
    import gaussian_scene as gs
    import synthetic
    P = 1500
    sc = synthetic.make_scene(P, C=3, tanfovx=0.6, tanfovy=0.6 * H / W, seed=0, logscale_mean=-4.0)
    s = gs.GaussianScene(xyz=sc.means3D, features_dc=sc.shs[:, :1].clone(), features_rest=sc.shs[:, 1:].clone(),
                         language_feature=sc.lang * 3.0, opacity=torch.logit(sc.opacities),
                         scaling=torch.log(sc.scales), rotation=sc.rotations).to("cuda")
    aabb = torch.stack([s.xyz.max(0).values, s.xyz.min(0).values]).cpu()
    p = DeformationField.init_params([12, 10, 9, 7], [1, 2], aabb, channels=32, width=64, heads=DNERF_HEADS, seed=5)
    g = torch.Generator().manual_seed(1)
    for k in p:                                                  # time planes of ones deform nothing over time
        if k.startswith("grid.grids"):
            p[k] = torch.rand(p[k].shape, generator=g) * 0.8 + 0.2
    s.deformation = DeformationField({k: v.cuda() for k, v in p.items()}, [12, 10, 9, 7], [1, 2], no_do=True,
                                     no_dshs=True)
    gs.save_model_dir(s, str(tmp_path), 7000, "fine-base")
    m, it = gs.load_model_dir(str(tmp_path), load_stage="fine-base")
    assert it == 7000 and (m.deformation.channels, m.deformation.width) == (32, 64)
    assert m.deformation.heads_computed() == list(DNERF_HEADS) and m.deformation.depth == 0
    t = torch.linspace(-1, 1, P, device="cuda")
    ins = (s.xyz, s.scaling, s.rotation, s.opacity, s.get_features, None, t)
    for a, b in zip(s.deformation.forward(*ins)[:5], m.deformation.forward(*ins)[:5]):
        assert torch.equal(a, b)
    cam = synthetic.origin_camera(W, H, 0.6)
    cam.time = 0.6
    bg = torch.ones(3, device="cuda")
    a, b = gs.render(cam, s, bg, stage="fine-base"), gs.render(cam, m, bg, stage="fine-base")
    assert torch.equal(a["render"], b["render"])
    assert not torch.equal(a["render"], gs.render(cam, s, bg, stage="coarse-base")["render"])


def test_two_training_steps_in_fine_base():
    """Two TrainStep iterations on a tiny synthetic scene with a dnerf-shaped field: every field
    parameter and gradient is finite and every computed module's parameters moved; capture() /
    restore() hand the field over; the discrete stage is refused."""
    import synthetic
    from gaussian_scene import render
    from gaussian_train import GaussianTrainer
    from train_step import TrainStep
    P = 1500
    dev = torch.device("cuda")
    sc = synthetic.make_scene(P, C=3, tanfovx=0.6, tanfovy=0.6 * H / W, seed=3, logscale_mean=-3.0).to(dev)
    cams = synthetic.camera_batch(2, W, H, tanfovx=0.6, seed=2)

    def raw():
        shs = sc.shs
        return {"xyz": sc.means3D.clone(), "f_dc": shs[:, :1].contiguous(), "f_rest": shs[:, 1:].contiguous(),
                "opacity": torch.logit(sc.opacities.reshape(P, 1)).contiguous(),
                "scaling": torch.log(sc.scales).contiguous(), "rotation": sc.rotations.clone()}

    field_p = DeformationField.init_params([8, 8, 8, 5], [1, 2], AABB, channels=32, width=64, heads=DNERF_HEADS, seed=1)
    mk = lambda: DeformationField({k: v.to(dev) for k, v in field_p.items()}, [8, 8, 8, 5], [1, 2], no_do=True,   # noqa: E731
                                  no_dshs=True)
    with torch.no_grad():
        tscene = TrainStep(GaussianTrainer(raw(), LRS), mk(), stage="fine-base").scene()
        gts = torch.stack([render(c, tscene, torch.ones(3, device=dev), stage="fine-base")["render"] for c in cams])
    r = raw()
    r["f_dc"] = r["f_dc"] + 0.5 * torch.randn(P, 1, 3, generator=torch.Generator().manual_seed(9)).to(dev)
    field = mk()
    step = TrainStep(GaussianTrainer(r, LRS), field, stage="fine-base")
    before = {k: v.clone() for k, v in field.p.items()}
    losses = [float(step(cams, gts)) for _ in range(2)]
    torch.cuda.synchronize()
    assert all(np.isfinite(x) for x in losses), losses
    for k, v in field.p.items():
        assert bool(torch.isfinite(v).all()), k
    for k, v in field.grads.items():
        assert bool(torch.isfinite(v).all()), k
    modules = {k.rsplit(".", 1)[0] if not k.startswith("grid.grids") else k for k in before if k != "grid.aabb"}
    for mod in modules:
        assert any(not torch.equal(field.p[k], before[k]) for k in before if k.startswith(mod)), mod
    cap = step.capture()
    other = TrainStep(GaussianTrainer(raw(), LRS), mk(), stage="fine-base")
    other.restore(cap)
    for k, v in field.p.items():
        assert torch.equal(other.field.p[k], v), k
    assert (other.field.channels, other.field.width) == (32, 64)
    import language_centers as lc
    with pytest.raises(ValueError, match="enter_discrete_stage.*32"):   # the discrete stage is the 16 / 128 field's
        lc.enter_discrete_stage(step)


def test_regularize_on_32_channel_planes():
    """field.regularize on 32-channel planes against the torch formulation of plane_regularizer.py in
    float64, within test_plane_reg_gpu.py's bounds (accumulated onto a seeded gradient)."""
    import plane_regularizer as pr
    from test_plane_reg_gpu import check_grad, check_total
    p = DeformationField.init_params(RES, [1, 2], [[1, 1, 1], [-1, -1, -1]], channels=32, width=64, heads=DNERF_HEADS)
    g = torch.Generator().manual_seed(2)
    for k in p:
        if k.startswith("grid.grids"):
            p[k] = torch.rand(p[k].shape, generator=g) * 1.5 + 0.1
    f = DeformationField({k: v.cuda() for k, v in p.items()}, RES, [1, 2], no_do=True, no_dshs=True)
    weights = (1e-2, 1e-4, 2e-4)
    f.zero_grad()
    prev = {}
    for k in f.grads:
        if k.startswith("grid.grids"):
            f.grads[k].copy_(torch.randn(f.grads[k].shape, generator=g) * 1e-3)
            prev[k] = f.grads[k].cpu().numpy().copy()
    res = f.regularize(weights)
    torch.cuda.synchronize()
    planes64 = [[p[f"grid.grids.{s}.{ci}"].double() for ci in range(6)] for s in range(2)]
    grads64 = [[torch.zeros_like(t) for t in s] for s in planes64]
    want = pr.regularize_planes_torch(planes64, weights, grads64, accumulate=False)
    n_elems = sum(t.numel() for s in planes64 for t in s)
    check_total(float(res.total), float(res.total64), float(want.total), n_elems, "32 channels")
    for s in range(2):
        for ci in range(6):
            k = f"grid.grids.{s}.{ci}"
            check_grad(f.grads[k].cpu().numpy(), grads64[s][ci].numpy(), prev=prev[k], what=k)
