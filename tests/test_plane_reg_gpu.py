"""The fused HexPlane regularisers (lsr_plane_reg, plane_regularizer.py, DeformationField.regularize,
TrainStep(plane_reg=...)) on the GPU.

Reference: the float64 numpy restatement of tests/plane_reg_cases.py on the same float32 inputs (held against the
REFERENCE's functions by tests/test_plane_reg.py), and tests/golden/plane_reg.npz for the whole field.

Tolerances, derived (N = C H W of the plane; for the total, the elements of all planes plus 3 for its own
weighting: two products and an add):
  loss terms           |x - x64| <= N 2^-53 x64: non-negative float64 sums, only their order differs
  gradient, overwrite  |g - g64| <= 2^-23 |g64|: one rounding to float32 (2^-24) and float64 order slack
  gradient, accumulate |out - (prev + g64)| <= 2^-23 |prev + g64| + 2^-24 |g64|: the float32 add on top
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import plane_reg_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plane_reg.npz")
DEV = "cuda"
GUARD = 64          # floats of canary on either side of every gradient buffer
CANARY = 12345.0


# ---- harness -------------------------------------------------------------------------------------------------------
def run_abi(planes, weights, prev=None, accumulate=False, with_grad=True, stream=None):
    """lsr_plane_reg on float32 planes [1, C, H, W] (numpy) with per-plane (w_smooth, w_l1).  with_grad: True, False,
    or one bool per plane.  Gradient buffers sit between canaries, which must come back intact.
    Returns (terms [n, 2], total32, total64, grads: numpy or None per plane)."""
    from diff_gaussian_rasterization import _lib
    L = _lib.load()
    n = len(planes)
    want = [with_grad] * n if isinstance(with_grad, bool) else list(with_grad)
    ts = [torch.from_numpy(np.ascontiguousarray(p)).to(DEV) for p in planes]
    bufs = []
    for i, p in enumerate(planes):
        b = torch.full((p.size + 2 * GUARD,), CANARY, device=DEV)
        if prev is not None:
            b[GUARD:GUARD + p.size] = torch.from_numpy(prev[i].reshape(-1)).to(DEV)
        bufs.append(b)
    desc = (_lib.PlaneDesc * max(n, 1))()
    for i, (t, (ws, wl)) in enumerate(zip(ts, weights)):
        d = desc[i]
        d.t = t.data_ptr()
        d.grad = bufs[i].data_ptr() + 4 * GUARD if want[i] else None
        _, d.C, d.H, d.W = planes[i].shape
        d.w_smooth, d.w_l1 = ws, wl
    nbytes = int(L.lsr_plane_reg_workspace_bytes(n, desc))
    assert nbytes >= 16, L.lsr_last_error()
    ws_buf = torch.full((nbytes // 8 + 2,), float("nan"), dtype=torch.float64, device=DEV)   # a guard pair behind it
    out = torch.full((2 * n + 2,), float("nan"), dtype=torch.float64, device=DEV)
    total32 = torch.full((1,), float("nan"), device=DEV)

    def call():
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(L.lsr_plane_reg(n, desc, int(accumulate), ws_buf.data_ptr(), out.data_ptr(), total32.data_ptr(),
                                   out.data_ptr() + 16 * n, st), "lsr_plane_reg")
    if stream is None:
        call()
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            call()
        torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.isnan(o[2 * n + 1]) and bool(torch.isnan(ws_buf[nbytes // 8:]).all())   # nothing past the outputs
    grads = []
    for i, p in enumerate(planes):
        b = bufs[i].cpu().numpy()
        assert np.all(b[:GUARD] == CANARY) and np.all(b[GUARD + p.size:] == CANARY), f"plane {i}: canary overwritten"
        inner = b[GUARD:GUARD + p.size].reshape(p.shape)
        if want[i]:
            grads.append(inner.copy())
        else:
            assert np.all(inner == (CANARY if prev is None else prev[i])), f"plane {i}: written without a gradient"
            grads.append(None)
    return o[:2 * n].reshape(n, 2).copy(), float(total32.item()), float(o[2 * n]), grads


def check_terms(terms, planes, what=""):
    for i, p in enumerate(planes):
        s64, a64 = pc.smooth_np(p)[0], pc.l1_np(p)[0]
        tol = p.size * 2.0 ** -53
        print(f"{what} plane {i} {p.shape}: smooth {terms[i, 0]!r} vs {s64!r}, l1 {terms[i, 1]!r} vs {a64!r}")
        assert abs(terms[i, 0] - s64) <= tol * s64, (what, i, terms[i, 0], s64)
        assert abs(terms[i, 1] - a64) <= tol * a64, (what, i, terms[i, 1], a64)


def check_total(total32, total64, want, n_elems, what=""):
    print(f"{what} total {total64!r} vs {want!r} (float32 {total32!r})")
    # the terms' bound, and one rounding each for the two products and the add of terms that differ that much
    assert abs(total64 - want) <= (n_elems + 3) * 2.0 ** -53 * abs(want), (what, total64, want)
    assert total32 == float(np.float32(total64))


def check_grad(g, g64, prev=None, what=""):
    g, g64 = np.asarray(g, np.float64), np.asarray(g64, np.float64)
    if prev is None:
        err, tol = np.abs(g - g64), 2.0 ** -23 * np.abs(g64)
    else:
        s = prev.astype(np.float64) + g64
        err, tol = np.abs(g - s), 2.0 ** -23 * np.abs(s) + 2.0 ** -24 * np.abs(g64)
    worst = float((err - tol).max())
    print(f"{what} gradient: worst error over tolerance {worst:.3e}, max |g64| {float(np.abs(g64).max()):.3e}")
    assert worst <= 0, (what, worst)


# ---- single planes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", pc.KINDS)
@pytest.mark.parametrize("mode", list(pc.MODES))
@pytest.mark.parametrize("shape", pc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_single_plane(shape, mode, kind):
    """Every shape smooth-only, L1-only and both, on spatial and on time values: overwriting, then accumulating
    onto a seeded non-zero gradient."""
    rng = np.random.default_rng(100 * pc.SHAPES.index(shape) + 10 * list(pc.MODES).index(mode) + pc.KINDS.index(kind))
    t = pc.plane_values(shape, kind, rng)
    ws, wl = pc.MODES[mode]
    s64, a64, g64 = pc.plane_np(t, ws, wl)
    terms, total32, total64, (g,) = run_abi([t], [(ws, wl)])
    check_terms(terms, [t], "overwrite")
    check_total(total32, total64, ws * s64 + wl * a64, t.size, "overwrite")
    check_grad(g, g64, what="overwrite")
    prev = (rng.normal(size=t.shape) * 1e-3).astype(np.float32)
    prev[prev == 0] = 1e-3
    terms2, _, total64b, (ga,) = run_abi([t], [(ws, wl)], prev=[prev], accumulate=True)
    assert np.array_equal(terms2, terms) and total64b == total64
    check_grad(ga, g64, prev=prev, what="accumulate")
    # the loss alone: the same bits, nothing written
    terms3, total32c, total64c, _ = run_abi([t], [(ws, wl)], prev=[prev], with_grad=False)
    assert np.array_equal(terms3, terms) and (total32c, total64c) == (total32, total64)


def test_linear_ramp_has_no_second_difference():
    """t[c, j, w] = 0.25 j + 0.5 c: every d2 is an exact 0, so are the term and the gradient."""
    C, H, W = 5, 9, 70
    t = (0.25 * np.arange(H)[None, :, None] + 0.5 * np.arange(C)[:, None, None] + np.zeros((1, 1, W)))
    t = t.astype(np.float32)[None]
    terms, total32, total64, (g,) = run_abi([t], [(1.0, 0.0)])
    assert terms[0, 0] == 0.0 and total64 == 0.0 and total32 == 0.0
    assert np.array_equal(g, np.zeros_like(g))
    assert terms[0, 1] > 0                                       # the L1 term is reported whatever its weight


def test_plane_of_ones_has_no_l1_gradient():
    t = np.ones((1, 16, 7, 33), np.float32)
    terms, total32, total64, (g,) = run_abi([t], [(0.0, 1.0)])
    assert np.array_equal(g, np.zeros_like(g)) and terms[0, 1] == 0.0 and total64 == 0.0
    terms, _, total64, (g,) = run_abi([t], [(1.0, 1.0)])         # a fresh time plane: both terms, still nothing
    assert np.array_equal(g, np.zeros_like(g)) and np.array_equal(terms, np.zeros((1, 2))) and total64 == 0.0


def test_short_plane_takes_the_l1_term_alone():
    """H < 3 with w_smooth == 0: no stencil, smooth reported as 0."""
    rng = np.random.default_rng(3)
    t = pc.plane_values((2, 2, 130), "time", rng)
    terms, _, total64, (g,) = run_abi([t], [(0.0, 0.5)])
    a64, ga = pc.l1_np(t)
    assert terms[0, 0] == 0.0 and abs(terms[0, 1] - a64) <= t.size * 2.0 ** -53 * a64
    check_grad(g, 0.5 * ga, what="H = 2")


def test_no_planes_is_a_zero_total():
    terms, total32, total64, grads = run_abi([], [])
    assert terms.shape == (0, 2) and total32 == 0.0 and total64 == 0.0 and grads == []


# ---- whole fields ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    d = {k: z[k] for k in z.files}
    d["planes"] = [[d[f"plane/{s}/{ci}"] for ci in range(6)] for s in range(2)]
    d["grads"] = [[d[f"grad/{s}/{ci}"] for ci in range(6)] for s in range(2)]
    return d


def _module_run(planes, weights, prev=None, accumulate=False, dtype=torch.float32):
    import plane_regularizer as pr
    ts = [[torch.from_numpy(p).to(DEV, dtype) for p in s] for s in planes]
    if prev is None:
        gs = [[torch.full_like(t, CANARY) for t in s] for s in ts]
    else:
        gs = [[torch.from_numpy(g).to(DEV, dtype) for g in s] for s in prev]
    res = pr.regularize_planes(ts, weights, gs, accumulate=accumulate)
    torch.cuda.synchronize()
    return res, gs


def test_golden_field_in_one_call(golden):
    """The 12 planes of the golden field through the module against the REFERENCE's numbers."""
    planes, W = golden["planes"], pc.GOLDEN_WEIGHTS
    n_elems = sum(p.size for s in planes for p in s)
    res, gs = _module_run(planes, W)
    assert res.total.is_cuda and res.total.dtype == torch.float32 and res.total.dim() == 0
    assert res.terms.dtype == torch.float64 and res.terms.shape == (12, 2)
    terms = res.terms.cpu().numpy()
    for i, (s64, a64) in enumerate(golden["terms"]):
        tol = planes[i // 6][i % 6].size * 2.0 ** -53
        assert abs(terms[i, 0] - s64) <= tol * s64 and abs(terms[i, 1] - a64) <= tol * a64, (i, terms[i], s64, a64)
    check_total(float(res.total), float(res.total64), float(golden["total"]), n_elems, "golden")
    for name in ("plane_smooth", "time_smooth", "time_l1"):
        got, want = float(getattr(res, name)), float(golden[name])
        assert abs(got - want) <= n_elems * 2.0 ** -53 * want, (name, got, want)
    for s in range(2):
        for ci in range(6):
            check_grad(gs[s][ci].cpu().numpy(), golden["grads"][s][ci], what=f"golden {s}.{ci}")
    # accumulate onto a seeded gradient
    rng = np.random.default_rng(9)
    prev = [[(rng.normal(size=p.shape) * 1e-3).astype(np.float32) for p in s] for s in planes]
    res2, gs2 = _module_run(planes, W, prev=prev, accumulate=True)
    assert torch.equal(res2.terms, res.terms) and torch.equal(res2.total, res.total)
    for s in range(2):
        for ci in range(6):
            check_grad(gs2[s][ci].cpu().numpy(), golden["grads"][s][ci], prev=prev[s][ci], what=f"golden+ {s}.{ci}")


def test_four_scale_field_in_one_call():
    """24 planes, the most one call takes: resolution [3, 3, 3, 3], multires [1, 2, 4, 8]."""
    rng = np.random.default_rng(24)
    shapes = pc.plane_shapes([3, 3, 3, 3], [1, 2, 4, 8])
    planes = [[pc.plane_values(sh, "time" if ci in pc.TIME else "spatial", rng) for ci, sh in enumerate(s)]
              for s in shapes]
    W = (1e-2, 1e-4, 1e-4)
    total64, terms64, grads64 = pc.field_np(planes, W)
    flat = [p for s in planes for p in s]
    terms, total32, total, grads = run_abi(flat, [pc.plane_weights(W, i % 6) for i in range(24)])
    check_terms(terms, flat, "24 planes")
    check_total(total32, total, total64, sum(p.size for p in flat), "24 planes")
    for i, g in enumerate(grads):
        check_grad(g, grads64[i // 6][i % 6], what=f"24 planes {i}")
    res, gs = _module_run(planes, W)                              # the module builds the same descriptors
    assert np.array_equal(res.terms.cpu().numpy(), terms) and float(res.total64) == total
    assert all(np.array_equal(gs[i // 6][i % 6].cpu().numpy(), grads[i]) for i in range(24))


def test_calls_repeat_bit_for_bit_on_any_stream(golden):
    flat = [p for s in golden["planes"] for p in s]
    w = [pc.plane_weights(pc.GOLDEN_WEIGHTS, i % 6) for i in range(12)]
    a = run_abi(flat, w)
    b = run_abi(flat, w)
    c = run_abi(flat, w, stream=torch.cuda.Stream())
    for other in (b, c):
        assert np.array_equal(a[0], other[0]) and a[1:3] == other[1:3]
        assert all(np.array_equal(x, y) for x, y in zip(a[3], other[3]))


def test_planes_without_a_gradient_buffer_are_left_alone(golden):
    """grad == NULL on some planes of a call: their (canary) buffers stay untouched, the others are written, the
    terms and the total are those of the full call; and the module's grads=None gives the same bits."""
    import plane_regularizer as pr
    flat = [p for s in golden["planes"] for p in s]
    w = [pc.plane_weights(pc.GOLDEN_WEIGHTS, i % 6) for i in range(12)]
    full = run_abi(flat, w)
    some = run_abi(flat, w, with_grad=[i % 3 != 1 for i in range(12)])      # run_abi asserts the canaries
    assert np.array_equal(full[0], some[0]) and full[1:3] == some[1:3]
    assert all(g is None if i % 3 == 1 else np.array_equal(g, full[3][i]) for i, g in enumerate(some[3]))
    ts = [[torch.from_numpy(p).to(DEV) for p in s] for s in golden["planes"]]
    res = pr.regularize_planes(ts, pc.GOLDEN_WEIGHTS)
    assert np.array_equal(res.terms.cpu().numpy(), full[0]) and float(res.total64) == full[2]


def test_other_inputs_take_the_torch_formulation(golden, monkeypatch):
    import plane_regularizer as pr
    monkeypatch.setattr(pr, "_native", lambda *a, **k: pytest.fail("the kernel was called"))
    res, gs = _module_run(golden["planes"], pc.GOLDEN_WEIGHTS, dtype=torch.float64)   # float64 on the GPU
    assert res.total.is_cuda and res.total.dtype == torch.float64
    assert abs(float(res.total) - float(golden["total"])) <= 1e-12 * float(golden["total"])
    g, want = gs[1][4].cpu().numpy(), golden["grads"][1][4]
    assert np.all(np.abs(g - want) <= 1e-12 * np.abs(want))
    ts = [[torch.from_numpy(p).to(DEV) for p in s] for s in golden["planes"]]
    assert pr.native_eligible([t for s in ts for t in s])
    ts[0][0] = ts[0][0].transpose(2, 3).contiguous().transpose(2, 3)                  # not contiguous
    assert not pr.native_eligible([t for s in ts for t in s])
    res = pr.regularize_planes(ts, pc.GOLDEN_WEIGHTS)
    assert abs(float(res.total) - float(golden["total"])) <= 1e-5 * float(golden["total"])


def test_compute_regulation_on_parameters(golden):
    """The drop-in for gaussians.compute_regulation(...) on nn.Parameter planes: a scalar with a grad_fn whose
    backward hands every plane grad_output times the fused call's gradient."""
    import plane_regularizer as pr
    planes = [[torch.nn.Parameter(torch.from_numpy(p).to(DEV)) for p in s] for s in golden["planes"]]
    tsw, l1w, tvw = pc.GOLDEN_WEIGHTS
    total = pr.compute_regulation(planes, tsw, l1w, tvw)
    assert total.is_cuda and total.dim() == 0 and total.grad_fn is not None
    want, gs = _module_run(golden["planes"], pc.GOLDEN_WEIGHTS)
    assert torch.equal(total.detach(), want.total)
    (2.0 * total).backward()                                       # a power of two: the scaling is exact
    for s in range(2):
        for ci in range(6):
            assert torch.equal(planes[s][ci].grad, 2.0 * gs[s][ci])


# ---- the field and TrainStep ---------------------------------------------------------------------------------------
AABB = [[7.0, 5.5, 10.5], [-7.0, -5.5, 1.5]]
RES, MULTIRES = [8, 8, 8, 6], [1, 2]
WEIGHTS = (1e-3, 1e-4, 2e-4)
LRS = {"xyz": 1.6e-4, "f_dc": 2.5e-2, "f_rest": 2.5e-2 / 20, "opacity": 0.05, "scaling": 5e-3, "rotation": 1e-3,
       "language_feature": 2.5e-3}
P, SIDE = 64, 32


def _field():
    from deformation import DeformationField
    p = DeformationField.init_params(RES, MULTIRES, AABB, seed=1)
    g = torch.Generator().manual_seed(2)
    for k, v in p.items():                                        # time planes a little off 1, half of them
        if k.startswith("grid.grids") and k[-1] in "245":
            hit = torch.rand(v.shape, generator=g) < 0.5
            p[k] = torch.where(hit, v + 1e-2 * torch.randn(v.shape, generator=g), v)
    return DeformationField({k: v.to(DEV) for k, v in p.items()}, RES, MULTIRES)


def _step(stage, **kw):
    """A TrainStep on 64 Gaussians that all lie behind the camera, one 32 x 32 view: nothing is rendered, so the
    render's gradient into the field is exactly zero and the field's float atomics cannot blur a comparison."""
    import synthetic
    from gaussian_train import GaussianTrainer
    from train_step import TrainStep
    sc = synthetic.make_scene(P, C=3, tanfovx=0.6, tanfovy=0.6, seed=3, logscale_mean=-3.0)
    sc.means3D[:, 2] *= -1.0
    sc = sc.to(DEV)
    raw = {"xyz": sc.means3D.contiguous(), "f_dc": sc.shs[:, :1].contiguous(), "f_rest": sc.shs[:, 1:].contiguous(),
           "opacity": torch.logit(sc.opacities.reshape(P, 1)).contiguous(), "scaling": torch.log(sc.scales).contiguous(),
           "rotation": sc.rotations.contiguous()}
    if "lang" in stage:
        raw["language_feature"] = sc.lang.contiguous()
    cams = [synthetic.origin_camera(SIDE, SIDE, tanfovx=0.6)]
    g = torch.Generator().manual_seed(11)
    sup = dict(gts=torch.rand(1, 4, SIDE, SIDE, generator=g).to(DEV))
    if "lang" in stage:
        sup.update(gt_lang=torch.rand(1, 3, SIDE, SIDE, generator=g).to(DEV),
                   lang_mask=(torch.rand(1, 1, SIDE, SIDE, generator=g) < 0.7).float().to(DEV))
    step = TrainStep(GaussianTrainer(raw, {k: LRS[k] for k in raw}), _field(), stage=stage, **kw)
    return step, cams, sup


def _run(step, cams, sup):
    loss, _ = step.forward_backward(cams, sup["gts"], gt_lang=sup.get("gt_lang"), lang_mask=sup.get("lang_mask"))
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in step.trainer.params.items() if p.grad is not None}
    grads.update({"field/" + k: v.detach().clone() for k, v in step.field.grads.items()})
    return loss.detach().clone(), grads


def _overwrite_gradient(field):
    import plane_regularizer as pr
    S = range(len(field.multires))
    planes = [[field.p[f"grid.grids.{s}.{ci}"] for ci in range(6)] for s in S]
    grads = [[torch.full_like(t, CANARY) for t in s] for s in planes]
    res = pr.regularize_planes(planes, WEIGHTS, grads, accumulate=False)
    return res, {f"field/grid.grids.{s}.{ci}": grads[s][ci] for s in S for ci in range(6)}


def test_field_regularize_adds_to_its_gradients():
    field = _field()
    assert not hasattr(field, "grads")
    want, g = _overwrite_gradient(field)
    res = field.regularize(WEIGHTS)                               # makes the zeroed buffers first
    assert torch.equal(res.total, want.total) and torch.equal(res.terms, want.terms)
    assert float(res.time_l1) > 0 and float(res.time_smooth) > 0 and float(res.plane_smooth) > 0
    for k, v in g.items():
        assert torch.equal(field.grads[k[len("field/"):]], v), k
    field.regularize(WEIGHTS)                                     # and adds: g + g is exact
    for k, v in g.items():
        assert torch.equal(field.grads[k[len("field/"):]], 2 * v), k
    assert float(field.grads["feature_out.0.weight"].abs().max()) == 0.0
    field.regularize(WEIGHTS, accumulate=False)
    assert torch.equal(field.grads["grid.grids.1.2"], g["field/grid.grids.1.2"])


def test_train_step_fine_base_adds_the_term():
    step, cams, sup = _step("fine-base", plane_reg=WEIGHTS)
    twin, _, _ = _step("fine-base")
    assert step.plane_reg_active and not twin.plane_reg_active
    loss, grads = _run(step, cams, sup)
    loss0, grads0 = _run(twin, cams, sup)
    want, g = _overwrite_gradient(step.field)
    assert set(grads) == set(grads0) and set(g) < set(grads)
    for k in grads:
        if k in g:
            assert float(grads0[k].abs().max()) == 0.0, k        # nothing rendered: the render's share is zero
            assert torch.equal(grads[k], g[k]), k
            assert float(g[k].abs().max()) > 0, k
        else:
            assert torch.equal(grads[k], grads0[k]), k
    terms = step.plane_reg_terms
    assert torch.equal(terms.total, want.total) and torch.equal(terms.terms, want.terms)
    assert twin.plane_reg_terms is None
    exact = float(loss0) + float(want.total64)
    ulp = float(np.spacing(np.float32(abs(float(loss)))))
    print(f"loss {float(loss)!r}, twin {float(loss0)!r} + total {float(want.total64)!r}")
    assert float(want.total64) > 0 and abs(float(loss) - exact) <= ulp, (float(loss), exact, ulp)
    # the hook on its own: the gradient onto fresh buffers, the total onto any loss
    step.field.zero_grad()
    out = step.add_plane_reg(torch.tensor(0.25, device=DEV))
    assert torch.equal(out, torch.tensor(0.25, device=DEV) + want.total)
    assert all(torch.equal(step.field.grads[k[len("field/"):]], v) for k, v in g.items())


def test_train_step_whole_iteration_with_plane_reg():
    """__call__ with the term: the planes move (Adam on the regulariser's gradient alone), the loss is returned."""
    step, cams, sup = _step("fine-base", plane_reg=WEIGHTS)
    before = {k: v.clone() for k, v in step.field.p.items()}
    loss = step(cams, sup["gts"], iteration=1)
    torch.cuda.synchronize()
    assert loss.dim() == 0 and bool(torch.isfinite(loss))
    assert not torch.equal(step.field.p["grid.grids.0.2"], before["grid.grids.0.2"])
    assert torch.equal(step.field.p["feature_out.0.weight"], before["feature_out.0.weight"])   # zero gradient


@pytest.mark.parametrize("stage,kw", [("fine-lang", {}), ("coarse-base", {}), ("coarse-lang", dict(joint_train=True))],
                         ids=["fine-lang-frozen", "coarse-base", "coarse-lang-joint"])
def test_train_step_skips_the_term_where_the_planes_do_not_train(stage, kw):
    step, cams, sup = _step(stage, plane_reg=WEIGHTS, **kw)
    twin, _, _ = _step(stage, **kw)
    assert step.plane_reg == WEIGHTS and not step.plane_reg_active
    step.field.regularize = lambda *a, **k: pytest.fail("the regulariser ran")
    loss, grads = _run(step, cams, sup)
    loss0, grads0 = _run(twin, cams, sup)
    assert torch.equal(loss, loss0) and step.plane_reg_terms is None
    assert set(grads) == set(grads0)
    for k in grads:
        assert torch.equal(grads[k], grads0[k]), k
        if k.startswith("field/grid.grids"):
            assert float(grads[k].abs().max()) == 0.0, k


def test_plane_reg_carries_over_into_the_discrete_stage():
    """language_centers.enter_discrete_stage hands the step's switches to the new step, this one included."""
    from language_centers import enter_discrete_stage
    step, _, _ = _step("fine-lang", plane_reg=WEIGHTS, joint_train=True)
    new = enter_discrete_stage(step, "fine-base", centers=3, generator=torch.Generator(device=DEV).manual_seed(1))
    assert new.stage == "fine-lang-discrete" and new.plane_reg == WEIGHTS and new.plane_reg_active
    plain, _, _ = _step("fine-lang")
    new = enter_discrete_stage(plain, "fine-base", centers=3, generator=torch.Generator(device=DEV).manual_seed(1))
    assert new.plane_reg is None and not new.plane_reg_active


def test_train_step_fine_lang_with_joint_train_adds_the_term():
    step, cams, sup = _step("fine-lang", plane_reg=WEIGHTS, joint_train=True)
    assert step.plane_reg_active
    loss, grads = _run(step, cams, sup)
    want, g = _overwrite_gradient(step.field)
    assert all(torch.equal(grads[k], v) for k, v in g.items())
    assert torch.equal(step.plane_reg_terms.total, want.total)
